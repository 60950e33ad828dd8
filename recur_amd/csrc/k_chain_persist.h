// k_chain_persist.h -- the BPTT chain, one launch: k_chain_persist with its constants and its sync block (included by
// kernels_chain.hip, which launches it).  Its 256 workgroups wait for one another: residency, seats, the bounded poll and
// the give-up are k_coop.h's and are described in DESIGN.md, "Launches whose workgroups wait for one another".
//
// All D steps of the chain in ONE launch (hidden 1024: 32 column tiles; up to 8 row tiles of
// 32 streams).  What a kernel boundary costs the launch-per-step form -- 1.5 us of boundary,
// 1.7 us until the first operand stage has landed from a cold L2, the W panel fetched again
// every step -- is most of its 8.9 us; here the 32 workgroups that work on one row tile all
// run on ONE XCD (each reads the XCD it runs on from HW_REG_XCC_ID and draws its column tile
// by a ticket on that XCD: with one workgroup per CU and 32 CUs per XCD every XCD gets exactly
// 32, whatever the dispatch order), so that a step's output rows travel producer -> consumer
// through that XCD's L2 (plain stores, drained; a plain flag word per producer wave; L1-
// bypassing `sc1` polls and LDS-DMA loads), and each row tile is split into two independent
// sub-chains of 16 streams whose steps ALTERNATE on the matrix pipe: while the 32 workgroups
// exchange sub-chain a's step t, they multiply sub-chain b's.  (A row tile's recurrences are
// independent per stream: E[t+1][s] = mask[t][s] . (E[t][s] W^T), recur-nn.c:338-376.)
//
// Workgroup = 8 waves.  Waves 4-7 (one per SIMD) only multiply: the workgroup's W panel
// (32 output columns x 1024 k) lives in their registers for the whole launch as MFMA B
// fragments (v_mfma_f32_16x16x4_f32; each wave a quarter of K: 128 VGPRs), the A operand --
// 16 error rows x 1024 k per sub-chain, 64 KB -- is read from LDS with conflict-free
// ds_read_b128 (16-byte chunk c of row m sits at position c ^ m).  Waves 0-3 do everything
// else for four of the 16 rows each: finish the previous half-step (sum the four K quarters
// from LDS, zero-row mask, RESQRT derivative, sum of squares, store the rows), publish, poll
// the 32 producers of their rows, and pull the next operand into LDS by LDS-DMA.  One
// s_barrier per half-step couples the two groups.  Every poll is bounded; a time-out or a
// surplus ticket raises the abort word (host-mapped), which the library checks at its next
// synchronisation and aborts on -- results are never silently wrong.
/* (PC_SUB, the streams per sub-chain, PC_RED_FLOATS and pc_lds_bytes: k_tiles.h -- the residency probe has the launch's footprint) */
/* s_sleep units (64 cycles) between the barrier and the first poll; the producers publish ~0.35 us after
 * the barrier and the flag is visible in the XCD's L2 ~0.2 us later.  Round 3 (20 steps of 1024 / 256,
 * us per chain): first poll after 16 / 18 / 22 / 24 / 26 / 32 units with gaps from K block 3 on =
 * 114 / 105 / 100.6 / 100.7 / 101.3 / 105. */
#ifndef PC_SLEEP0
#define PC_SLEEP0 22
#endif
#ifndef PC_SLEEP0_ONE
#define PC_SLEEP0_ONE 12 /* 16-stream row tiles: the publish comes in an otherwise empty half-step */
#endif
#ifndef PC_SLEEP0_SMALL
#define PC_SLEEP0_SMALL 14 /* hidden 512 / 256: the half-step is shorter, the publish comes at the same ~0.35 us */
#endif
constexpr unsigned PC_EPOCH = COOP_CHAIN_EPOCH; /* flag values per launch (depth <= 60) */
/* K blocks (8 MFMAs each) after which the multiplying waves pause for 64 cycles, per hidden size:
 * measured at 1024: after blocks 3-6 100.6 us per chain, 3-7 100.8, 4-7 100.7, 3-8 100.9, 2-6 105.5,
 * 2-9 104.6, every block from 3 on 109.9, blocks 5 / 7 / 9 / 11 103.6-105.1, none (the poll then
 * completes when the burst has ended) 133. */
#ifndef PC_GAPS
#define PC_GAPS 0x78
#endif
#ifndef PC_GAPS_512
#define PC_GAPS_512 0x3c
#endif
#ifndef PC_GAPS_256
#define PC_GAPS_256 0xe
#endif
/* (Tried as build switches and retired, none faster: foreign MFMAs in the drain window -- profiles/r03_fused_delta_negative.txt;
 * a scalar poll of the flag words, s_nop gaps instead of s_sleep, s_setprio 3 around the fetch, ONE's fetching waves
 * fetching all of their rows themselves -- profiles/NOTES_r01_r03_design_diary.md, round 3, "133 -> 100.6 us".) */

struct ChainSync {
  unsigned tickets[8];       /* per XCD, monotonic over launches                     */
  unsigned pad0[24];
  unsigned flags[32][2][4][32]; /* [row tile][sub-chain][fetching wave][column tile]   */
  unsigned abort;            /* raised by any workgroup that gives up                */
};

#ifdef PC_STAMPS /* development builds only (tools/mkabl.sh -DPC_STAMPS): where a half-step's time goes */
__device__ unsigned long long g_pc_stamps[2][64][8];
#define PC_STAMP(role, k, slot)                                                                    \
  do {                                                                                             \
    if (g == 0 && j == 0 && lane == 0 && (wave8 & 3) == 0 && (k) < 64)                             \
      g_pc_stamps[role][k][slot] = __builtin_amdgcn_s_memrealtime();                               \
  } while (0)
#else
#define PC_STAMP(role, k, slot) do { } while (0)
#endif

/* The top layer's weight delta in the chain launch's first microseconds (HoWork, k_common.h): 22 MFLOP that as
 * a launch of their own (k_gemm<ProbHoDelta>) cost 6 us of launch, ramp and three dependent memory round trips
 * on the generation's critical path.  Here the launch's workgroups share the rows of the delta, HR =
 * ceil(H / workers) each: all 256 of them before they request their weight panel / while their first operand
 * rows are in flight, or -- when at least half of the launch has no chain work, a small set -- only those
 * (hw.idle_only; the others start their chain at once).  Lane (output quad q4, group gl) of wave w sums
 * streams g = 4 w + gl, g + 32, ... for ALL HR rows: one float4 of o_error and HR hidden values per stream (a
 * thread per row instead had five lanes load every float4 again, and the texture path is paid by the lane:
 * 3.6 us, now 2.5).  The four groups of a wave are added by shuffles, the eight waves in order through LDS
 * (`lds`: 8 x HO_HR x 64 floats the caller does not need yet: the partial-tile area, which is unused until the
 * first multiply has finished, or the operand buffers of a workgroup without chain work).  A workgroup's 512
 * threads all call it, once (two barriers). */
/* (chain_ho_sum / chain_ho_delta: k_common.h -- the weight-delta launch of the fused text step runs them too) */
/* ONE: row tiles of 16 streams, i.e. only sub-chain a exists and every other half-step is empty
 * (the workgroup multiplies, then finishes and publishes, then waits for the 32 producers of its
 * next operand): 4.5 instead of 6.4 us per step for HALF the streams per workgroup -- worse per
 * stream, but a small set (64 streams at hidden 1024: a GPU's share of 512 on eight) then runs
 * on twice as many CUs.  The launcher picks it when the 16-stream tiles still fit one launch. */
/* PAD (with ONE): the set is not whole row tiles -- only rows [vlo, nvalid) of the launch are its
 * own; the others belong to other streams or to nobody: they are multiplied like the rest (rows
 * do not mix) and never stored. */
template <int ACT, int K, bool ONE = false, bool PAD = false, bool XD = false> /* rnn_activation; hidden size: 1024, 512 or 256; XD: the tail for DENSE inputs (an instantiation of its own: the text step's kernel stays what it is) */
__global__ __launch_bounds__(512) void k_chain_persist(const View *__restrict__ vp, int uniform_idx,
                                                       int row0, int nrows, int depth, unsigned seq,
                                                       ChainSync *sy, unsigned *host_abort, int nvalid, int vlo,
                                                       HoWork hw, XcWork xc, int static_map, unsigned tseq, const unsigned *seats) {
  /* above the noise generator's waves (priority 0), which share four SIMDs with workgroups of this launch while the set
   * has presynaptic noise: the launch runs at the pace of its slowest workgroup (multi-head step, 256 / 32 streams:
   * 369 -> 360 / 221 -> 218 us per generation; nothing else changes) */
  __builtin_amdgcn_s_setprio(2);
  /* (first: one scalar load beside the arguments' -- k_coop.h: seat_tbl_p) */
  const unsigned hw_xcc = coop_hw_xcc();
  const unsigned hw_seat = static_map == 2 ? coop_seat(seats, hw_xcc) : 0u;
  extern __shared__ __attribute__((aligned(16))) float psm[];
  constexpr int BUF = PC_SUB * K;             /* one sub-chain's operand (64 KB at K = 1024) */
  constexpr int NT = K / 32;                  /* column tiles of a row tile            */
  constexpr int KB = K / 64;                  /* 16-k blocks of a wave's K quarter     */
  constexpr int PPR = K / 256;                /* 1 KB LDS-DMA pieces per operand row   */
  float *abuf = psm;                          /* [2][16][K], swizzled chunks           */
  float *red = psm + 2 * BUF;                 /* [2][4 waves][16 rows][32 cols]        */
  unsigned *wg_info = reinterpret_cast<unsigned *>(red + 2 * PC_RED_FLOATS);
  XC_STAMP(0);
  BND_MARK(g_bnd_chain, 0);
  PRO_STAMP_DEP(16, 256, nrows);        /* the launch's arguments are here */
  PRO_STAMP_DEP(17, 256, (int)hw_seat); /* the seat */
  View v = *vp;
  PRO_STAMP_DEP(18, 256, v.sh.H);       /* the view */
  v.b.uniform_idx = uniform_idx;
  const RamdShape &s = v.sh;
  const int wave8 = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int TR = ONE ? PC_SUB : 2 * PC_SUB; /* streams of a row tile */
  const int mtiles = nrows / TR;

  // --- which XCD am I on, and which of its 32 seats do I get.  static_map (the process's residency probe found the
  // launch's workgroups dealt to the XCDs in turn, workgroup i on XCD i % 8: coop_rule.h): XCD and seat follow
  // from the workgroup number, no ticket, no barrier -- each wave checks its XCD against the register, and a
  // mismatch gives the launch up (never silently wrong).  Otherwise: a ticket on the XCD the workgroup finds itself on.
  unsigned seat, my_xcc;
  if (static_map == 2) {
    /* the seat of the CU this workgroup runs on (one workgroup per CU: 137 KB of LDS): whatever order the dispatcher
     * dealt the workgroups in, and whatever else it dealt between them -- no atomic, no barrier, one scalar load */
    my_xcc = hw_xcc;
    seat = hw_seat;
  } else if (static_map) {
    my_xcc = blockIdx.x & 7u;
    seat = blockIdx.x >> 3;
    if (coop_hw_xcc() != my_xcc) seat = 32u;
  } else {
    if (threadIdx.x == 0) {
      const unsigned xcc = coop_hw_xcc();
      const unsigned t = __hip_atomic_fetch_add(&sy->tickets[xcc], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) -
                         (tseq - 1u) * 32u; /* (tseq: this launch's number among those that draw tickets) */
      wg_info[0] = xcc;
      wg_info[1] = t;
    }
    __syncthreads();
    /* (wave-uniform by construction: say so, or every address built from them goes through the vector ALU) */
    seat = __builtin_amdgcn_readfirstlane(wg_info[1]);
    my_xcc = __builtin_amdgcn_readfirstlane(wg_info[0]);
  }
  /* row tile = XCD + 8 x (seat / column tiles): the first 8 row tiles spread over the 8 XCDs
   * before any XCD takes a second one; column tile = seat % column tiles */
  const int g = (int)my_xcc + 8 * (int)(seat / NT);
  if (seat >= 32u) { /* cannot happen with one workgroup per CU on a 256-CU part */
    if (threadIdx.x == 0) coop_give_up(&sy->abort, host_abort, COOP_ABORT_CHAIN_OFF_XCD);
    return; /* (the launcher repeats the call's work another way, the top layer's delta included) */
  }
  if (g >= mtiles) { /* fewer row tiles than seats: no chain work here, only a share of the top layer's delta */
    if (hw.dst && hw.idle_only) {
      /* a small set: the workgroups without chain work share the rows among themselves (the others start their
       * chain at once).  Rank among them from (XCD, seat): XCD x' has its row-tile slots r0(x') .. SP - 1 idle. */
      constexpr int SP = 32 / NT; /* row-tile slots of an XCD */
      const int x = (int)my_xcc;
      auto r0 = [&](int xx) { const int r = (mtiles - xx + 7) / 8; return r < 0 ? 0 : r > SP ? SP : r; };
      int rank = (int)seat - r0(x) * NT;
      for (int xx = 0; xx < x; xx++) rank += (SP - r0(xx)) * NT;
      chain_ho_delta<9, 4>(v, hw, psm, rank);
    } else if (hw.dst) {
      chain_ho_delta<5, HO_BATCH>(v, hw, red, (int)blockIdx.x);
    }
    return;
  }
  const bool ho_here = hw.dst && !hw.idle_only; /* (kernel arguments: the same for every thread) */
  const int j = (int)(seat % NT);
  const int m0 = TR * g, n0 = 1 + 32 * j;     /* output columns start at 1 */
  const unsigned epoch0 = seq * PC_EPOCH;
  const int halfsteps = 2 * depth;
  const int tn = NT;
  const size_t plane_stride = (size_t)s.Scap * s.I;
  /* the tail's first stream (row tile's stream j): what it can ask for now (extras_tail_prefetch) */
  const bool xc_first = !XD && xc.on && j < TR && !(PAD && (m0 + j < vlo || m0 + j >= nvalid));
  TailPre tpre;
  PRO_STAMP(19, 256);
  if (xc_first) tpre = extras_tail_prefetch<512>(v, row0 + m0 + j, row0 + m0 + j - xc.row0, xc.nx, xc.active);
  PRO_STAMP(20, 256);

  if (wave8 >= 4) {
    // ============================================ multiply, finish, publish
    // Waves 4-7, one per SIMD.  Wave wv multiplies the K quarter wv of BOTH 16 x 16 tiles of
    // every half-step and, after the barrier, finishes rows 4 wv .. 4 wv + 3 of the tile
    // pair: the four K quarters summed from LDS, the zero-row mask, the RESQRT derivative, the
    // store, and -- once the stores have drained -- the flag that the 32 consumers of those rows
    // poll.  (The f32 MFMA runs on the SIMD's vector ALU at the vector rate: a partner wave's VALU
    // work does not overlap with it, so the epilogue belongs in the wave that owns the ALU.)
    //
    // Round 3: everything between the barrier and the flag is on the critical path of all 32
    // consumers, so it is written instruction by instruction:
    //   * the row stores, the gate loads and the flag go through an SGPR base + a launch-invariant
    //     per-lane byte offset (inline asm, `global_*` with saddr): no 64-bit address arithmetic,
    //     no register arrays indexed by the sub-chain (hipcc had turned those into a dozen
    //     v_cndmask per store and FLAT stores);
    //   * the flag is a PLAIN store (it stays in this XCD's L2, where the consumers' L1-bypassing
    //     polls find it).  As a `volatile` store hipcc made it `sc0 sc1` and put an
    //     `s_waitcnt vmcnt(0)` BEHIND it (SIMemoryLegalizer's rule for volatile accesses): every
    //     half-step waited a second time, for the flag's own acknowledgement, before its MFMAs;
    //   * the sum of squares of each error row (recur-nn.c:371) is no longer taken here (two
    //     multiplies, ten LDS-crossbar shuffles in five dependent round trips and two more stores
    //     in front of the drain): k_extras_control holds every error row in registers anyway and
    //     sums it there (tn = 0 in its arguments);
    //   * the A fragments come from LDS by inline-asm ds_read_b128 three K blocks ahead of the
    //     MFMAs that use them, with counted lgkmcnt waits (hipcc's own schedule had half of the
    //     sixteen reads directly in front of their first MFMA: 60-100 cycles of idle matrix pipe
    //     each), the first three before the finish, whose drain covers their latency.
    const int wv = __builtin_amdgcn_readfirstlane(wave8) - 4, m = lane & 15, kq = lane >> 4;
    const int col = lane & 31, rh = lane >> 5;
    if (ho_here) chain_ho_delta<5, HO_BATCH>(v, hw, red, (int)blockIdx.x); /* before the panel's loads: its own loads need the registers, and return first */
    PRO_STAMP(11, 256);
    float wreg[KB][4][2];
    {
      const float *wb = v.b.ih_w + (size_t)(n0 + m) * s.H + 1 + (K / 4) * wv + 4 * kq;
#pragma unroll
      for (int u = 0; u < KB; u++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int h = 0; h < 2; h++) wreg[u][i][h] = wb[(size_t)16 * h * s.H + 16 * u + i];
      PRO_STAMP(12, 256);
      /* The panel has to have LANDED before the loop, as far as hipcc can tell: otherwise it puts the
       * `s_waitcnt vmcnt(0)` for these loads in front of the loop's first MFMA, where it waits in EVERY
       * half-step for the gate loads issued just before (inline asm, not on its scoreboard).  An empty
       * asm that reads the registers makes it wait here. */
#pragma unroll
      for (int u = 0; u < KB; u++)
        asm volatile("" : : "v"(wreg[u][0][0]), "v"(wreg[u][0][1]), "v"(wreg[u][1][0]), "v"(wreg[u][1][1]),
                     "v"(wreg[u][2][0]), "v"(wreg[u][2][1]), "v"(wreg[u][3][0]), "v"(wreg[u][3][1]));
      PRO_STAMP(13, 256);
    }
    // this thread's two outputs per half-step: rows 4 wv + rh and + 2 of the sub-chain, column
    // n0 + col.  Byte offset of (row, column) within a plane of [Scap][I] floats, relative to
    // the sub-chain's first row: the same for the error planes and the history slots.
    unsigned voff[2];
    bool mine[2][2]; /* PAD: is the row one of the set's own */
#pragma unroll
    for (int q = 0; q < 2; q++) {
      voff[q] = (unsigned)(((size_t)(4 * wv + rh + 2 * q) * s.I + n0 + col) * sizeof(float));
#pragma unroll
      for (int x = 0; x < 2; x++) {
        const int sr = m0 + PC_SUB * x + 4 * wv + rh + 2 * q;
        mine[x][q] = !PAD || (sr >= vlo && sr < nvalid);
      }
    }
    const float *ehi_sub = v.b.ehi + (size_t)(row0 + m0) * s.I; /* plane 0, sub-chain a, row 0 */
    /* ONE: in the half-step that multiplies nothing this wave fetches the second half of its row group's
     * pieces of the next operand itself (rows 4 wv + 2, + 3 at K = 1024), the fetching wave the first half:
     * sixteen LDS-DMA instructions per wave took 0.4 us to issue, on the critical path of every step */
    unsigned hvoff[ONE ? 2 * PPR : 1];
    if constexpr (ONE) {
#pragma unroll
      for (int i = 0; i < 2 * PPR; i++) {
        const int ii = 2 * PPR + i, r = 4 * wv + ii / PPR;
        const int c = (64 * (ii % PPR) + lane) ^ r;
        hvoff[i] = (unsigned)(((size_t)r * s.I + 1 + 4 * c) * sizeof(float));
      }
    }
    // LDS addresses.  A fragment of K block u: chunk ((K / 16) wv + 4 u + kq) ^ m of row m; the
    // xor only touches the low four bits, i.e. (4 (u & 3) + kq) ^ m: four per-lane addresses per
    // sub-chain, the rest of u is an immediate offset.
    uint32_t a_addr[2][4];
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
      for (int i = 0; i < 4; i++)
        a_addr[x][i] = lds_byte_addr(abuf + x * BUF + m * K) + 16u * (uint32_t)((K / 16) * wv + ((4 * i + kq) ^ m));
    const uint32_t red_rd = lds_byte_addr(red) + 4u * (uint32_t)((4 * wv + rh) * 32 + col);
    float xg0 = 0.f, xg1 = 0.f;
    f32x4 af[4];
    bool mdead = false; /* somebody gave up: no more polling, only the barriers */
    __syncthreads(); /* barrier 0: both operands of the first two half-steps have landed */
    PRO_STAMP(14, 256);
    PRO_CLOCKS(24, 256);

    // one half-step; XC: which sub-chain it MULTIPLIES (it finishes the other one's previous half-step)
    auto half = [&](auto XC, const int k) -> bool {
      constexpr int x = decltype(XC)::value, xf = x ^ 1;
      const bool multiplies = k < halfsteps && !(ONE && x == 1);
      PC_STAMP(0, k, 0);
      if (multiplies) { /* the first fragments: their latency hides under the finish */
        af[0] = lds_read_b128_off<0>(a_addr[x][0]);
        if (KB > 1) af[1] = lds_read_b128_off<0>(a_addr[x][1]);
        if (KB > 2) af[2] = lds_read_b128_off<0>(a_addr[x][2]);
      }
      if (k >= 1 && !(ONE && x == 0)) {
        // ---- finish half-step k - 1 (sub-chain xf, step (k - 1) >> 1)
        const int t = (k - 1) >> 1;
        float ev[2];
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(xg0), "+v"(xg1)); /* the gate loads of the last half-step */
        {
          const uint32_t ra = red_rd + 4u * (uint32_t)(xf * PC_RED_FLOATS);
          float p[2][4];
#pragma unroll
          for (int q = 0; q < 2; q++) {
            p[q][0] = q ? lds_read_b32_off<256 + 0 * 2048>(ra) : lds_read_b32_off<0 * 2048>(ra);
            p[q][1] = q ? lds_read_b32_off<256 + 1 * 2048>(ra) : lds_read_b32_off<1 * 2048>(ra);
            p[q][2] = q ? lds_read_b32_off<256 + 2 * 2048>(ra) : lds_read_b32_off<2 * 2048>(ra);
            p[q][3] = q ? lds_read_b32_off<256 + 3 * 2048>(ra) : lds_read_b32_off<3 * 2048>(ra);
          }
          asm volatile("s_waitcnt lgkmcnt(0)"
                       : "+v"(p[0][0]), "+v"(p[0][1]), "+v"(p[0][2]), "+v"(p[0][3]), "+v"(p[1][0]), "+v"(p[1][1]),
                         "+v"(p[1][2]), "+v"(p[1][3]));
          ev[0] = (p[0][0] + p[0][1]) + (p[0][2] + p[0][3]);
          ev[1] = (p[1][0] + p[1][1]) + (p[1][2] + p[1][3]);
        }
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const float xi = q ? xg1 : xg0;
          const bool on = xi != 0.0f && (ACT != 5 || xi < 20.0f);
          ev[q] = on ? ev[q] : 0.0f;
          if (ACT == 2) ev[q] = on ? ev[q] / (2 * (xi + 1.0f)) : 0.0f;
        }
        const float *obase = ehi_sub + (size_t)(t + 1) * plane_stride + (size_t)xf * PC_SUB * s.I;
        if (mine[xf][0]) g_store_saddr(voff[0], ev[0], obase);
        if (mine[xf][1]) g_store_saddr(voff[1], ev[1], obase);
        PC_STAMP(0, k, 2);
        /* Drain and publish BEFORE the next MFMAs, with the vector ALU idle.  Every way of hiding
         * this wait under the multiply was slower (round 2: stores waited for 8 / 16 / 48 MFMAs
         * later 135 / 136 / 147 us per chain against 135; the finished tile handed through LDS to
         * the fetching waves 150-155 us; wave groups of their own per sub-chain 195 us): beside a
         * wave that issues f32 MFMAs back to back a store's acknowledgement comes 1-4 us late. */
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) g_store_saddr(0u, __uint_as_float(epoch0 + (unsigned)t + 1u), &sy->flags[g][xf][wv][j]);
        PC_STAMP(0, k, 3);
      }
      if (k == halfsteps) return false; /* nothing left to multiply (nobody polls the last flag) */
      if (!multiplies) {                /* ONE: sub-chain b does not exist, an empty half-step */
        if constexpr (ONE) {
          if (k >= 1 && k + 1 < halfsteps) {
            /* the flags of this wave's row group (the same ones its fetching wave polls), then its pieces */
            const unsigned want = epoch0 + (unsigned)((k - 1) >> 1) + 1u;
            const char *fbase = uniform_ptr(&sy->flags[g][0][wv][0]);
            const unsigned poff = (unsigned)((lane % NT) * sizeof(unsigned));
            /* (the fetching waves raise the alarm; this wave only heeds it) */
            if (!mdead) coop_poll(fbase, poff, want, &sy->abort, [&]() { mdead = true; });
            const char *base = uniform_ptr(ehi_sub + (size_t)((k + 1) >> 1) * plane_stride);
            const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_byte_addr(abuf + 4 * wv * K));
#pragma unroll
            for (int i = 0; i < 2 * PPR; i++) {
              const int ii = 2 * PPR + i;
              lds_dma16_sc1(base, hvoff[i], dst + (uint32_t)(((ii / PPR) * K + 256 * (ii % PPR)) * sizeof(float)));
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
        }
        __syncthreads();
        return true;
      }
      { /* the gate values X[t][row][n0 + col] for the finish of THIS half-step, one barrier from now */
        const float *gbase = input_row<true>(v, row0 + m0 + PC_SUB * x, k >> 1);
        xg0 = g_load_saddr(voff[0], gbase);
        xg1 = g_load_saddr(voff[1], gbase);
      }
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      static_for<KB>([&](auto UC) {
        constexpr int u = decltype(UC)::value;
        constexpr int ahead = KB - 1 - u < 2 ? KB - 1 - u : 2; /* reads issued after this block's */
        lgkm_wait<ahead>(af[u & 3]);
        if (u + 3 < KB) af[(u + 3) & 3] = lds_read_b128_off<((u + 3) >> 2) * 256>(a_addr[x][(u + 3) & 3]);
        const f32x4 a = af[u & 3];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wreg[u][0][0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wreg[u][0][1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wreg[u][1][0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wreg[u][1][1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wreg[u][2][0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wreg[u][2][1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wreg[u][3][0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wreg[u][3][1], acc1, 0, 0, 0);
        /* a short pause of the MFMA stream (64 cycles asleep = the last MFMA's 32 + 32 with the vector ALU
         * free): the fetching wave's one v_cmp per poll gets through here and nowhere else */
        if (!ONE && (((K == 1024 ? PC_GAPS : K == 512 ? PC_GAPS_512 : PC_GAPS_256) >> u) & 1)) { /* (ONE: nobody polls beside a burst) */
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_sleep(1);
          __builtin_amdgcn_sched_barrier(0);
        }
      });
      /* this wave's K quarter of the 16 x 32 tile: register r of the accumulator is row
       * 4 (lane >> 4) + r, column lane & 15 (+ 16 for the second accumulator) */
      /* (plain stores: hipcc knows how many wait states an MFMA result needs before an LDS write may
       * read it -- an inline-asm ds_write directly behind the last MFMA read the OLD accumulator) */
      {
        float *rdw = red + x * PC_RED_FLOATS + wv * (PC_SUB * 32);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          rdw[(4 * kq + r) * 32 + m] = acc0[r];
          rdw[(4 * kq + r) * 32 + 16 + m] = acc1[r];
        }
      }
      PC_STAMP(0, k, 1);
      __syncthreads(); /* barrier k + 1 */
      return true;
    };
    for (int k = 0;; k += 2) {
      if (!half(std::integral_constant<int, 0>{}, k)) break;
      if (!half(std::integral_constant<int, 1>{}, k + 1)) break;
    }
  } else {
  // ======================================================= poll and fetch
  // Waves 0-3: rows 4 lw .. 4 lw + 3 of each sub-chain's operand.  Almost no vector-ALU
  // work (one compare per poll), so the multiplying waves keep the ALU.
  const int lw = __builtin_amdgcn_readfirstlane(wave8); /* scalar: LDS addresses stay off the vector ALU */
  const int col = lane & 31, rh = lane >> 5;
  bool dead = false;                  /* gave up: keep the barriers going, nothing else */

  // fetch rows 4 lw .. + 3 of sub-chain x, error plane `plane`, into its LDS image: 16 pieces
  // of 1 KB (lane l of piece q lands at chunk position 64 (q & 3) + l of row q >> 2 and
  // therefore brings chunk position ^ row)
  // Per-lane BYTE offsets within a plane are fixed for the whole launch (the same for both
  // sub-chains: b's rows are 16 rows further on); the plane / sub-chain base is wave-uniform.
  // A fetch is then 16 x (s_mov m0, global_load_lds saddr + voffset): no vector-ALU
  // instruction, which beside a multiplying wave would wait for a gap in its MFMAs.
  unsigned voff[4 * PPR]; /* this wave's four rows, PPR pieces of 64 chunks each */
#pragma unroll
  for (int i = 0; i < 4 * PPR; i++) {
    const int r = 4 * lw + i / PPR;
    const int c = (64 * (i % PPR) + lane) ^ r;
    voff[i] = (unsigned)(((size_t)r * s.I + 1 + 4 * c) * sizeof(float));
  }
  const float *sub_base = v.b.ehi + (size_t)(row0 + m0) * s.I; /* plane 0, sub-chain a, row 0 */
  /* (Round 3, measured and removed: every workgroup of a row tile starting its fetch at another row and
   * piece, so that the NT CUs do not all ask the L2 for the same line at the same moment: 102.2 against
   * 100.8 us per chain, and the sixteen instructions still took 1.1-1.25 us to issue beside the burst.) */
  auto fetch = [&](int x, int plane, bool first_half_only = false) {
    const char *base = reinterpret_cast<const char *>(sub_base + (size_t)plane * plane_stride +
                                                      (size_t)x * PC_SUB * s.I);
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_byte_addr(abuf + x * BUF + 4 * lw * K));
#pragma unroll
    for (int i = 0; i < 4 * PPR; i++)
      if (i < 2 * PPR || !first_half_only) /* (ONE: the multiplying wave of the row group fetches the other half) */
        lds_dma16_sc1(base, voff[i], dst + (uint32_t)(((i / PPR) * K + 256 * (i % PPR)) * sizeof(float)));
  };
  // wait until all NT column tiles have published step t of sub-chain x (rows of this wave).
  // Beside a wave that issues f32 MFMAs back to back this wave gets NO vector-ALU instruction through
  // (round 3, once the multiplying waves' own stalls were gone: the twelve VALU instructions of the
  // compiler's poll loop completed only when the 128-MFMA burst had ended, stamps: flags published
  // 0.4 us after the barrier, "seen" at 2.5 us).  So the poll (coop_poll, k_coop.h) is one L1-bypassing vector load per
  // lane and ONE v_cmp, which takes the next of the short gaps that the multiplying waves leave in their MFMA stream
  // for exactly this (PC_GAPS).
  const unsigned poll_off = (unsigned)((lane % NT) * sizeof(unsigned));
  auto wait_for = [&](int x, int t) {
    const unsigned want = epoch0 + (unsigned)t + 1u;
    const unsigned *fbase = &sy->flags[g][x][lw][0];
    __builtin_amdgcn_s_sleep(ONE ? PC_SLEEP0_ONE : K == 1024 ? PC_SLEEP0 : PC_SLEEP0_SMALL);
    if (!coop_poll(fbase, poll_off, want, &sy->abort)) { /* has somebody else given up; have we been here for ~1 s */
      if (lane == 0) coop_give_up(&sy->abort, host_abort, COOP_ABORT_CHAIN);
      dead = true;
    }
  };

  fetch(0, 0);
  if (halfsteps > 1 && !ONE) fetch(1, 0);
  if (ho_here) chain_ho_delta<5, HO_BATCH>(v, hw, red, (int)blockIdx.x); /* while the first operand rows are on their way */
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PRO_STAMP(15, 0);
  __syncthreads(); /* barrier 0 */
  for (int k = 0; k < halfsteps; k++) {
    PC_STAMP(1, k, 0);
    if (k >= 1 && k + 1 < halfsteps && !dead && !(ONE && (k & 1) == 0)) {
      /* half-step k + 1 continues the sub-chain of half-step k - 1, which the multiplying
       * waves of all 32 column tiles are finishing right now */
      wait_for((k - 1) & 1, (k - 1) >> 1);
      PC_STAMP(1, k, 2);
      if (!dead) fetch((k + 1) & 1, (k + 1) >> 1, ONE);
      PC_STAMP(1, k, 3);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PC_STAMP(1, k, 4);
    __syncthreads(); /* barrier k + 1 */
  }
  }

  // ================================================ tail: the extras and the control logic
  // (XcWork, k_common.h.)  Stream i of the row tile belongs to column tile i % NT: at hidden 1024 with
  // 32-stream tiles every workgroup has exactly one.  A stream's rows of ALL error planes must have been
  // published by all NT column tiles: the flags of its row group at the last step (earlier ones were
  // raised before it, in program order behind a drained store queue) -- and only the item of the last
  // plane has to wait for them: every earlier plane was seen complete by this workgroup's own fetching
  // waves before a barrier that all its waves have passed.  The rows are read past the L1 (sc1 loads) from
  // this XCD's L2, where the row tile's planes were written.
  if (!xc.on) return;
  XC_STAMP(1);
  XC_STAMP(10);
  PRO_CLOCKS(26, 256);
  /* (the sums' scratch is the operand area: nobody reads it behind the loop's last barrier, while the
   * multiplying waves' last finish still reads `red` -- no barrier in front of the tail) */
  for (int i = j; i < TR; i += NT) {
    const int sr = m0 + i; /* row within the launch */
    if (PAD && (sr < vlo || sr >= nvalid)) continue; /* (kernel arguments and the seat: uniform over the workgroup) */
    const int x = i / PC_SUB, rg = (i % PC_SUB) >> 2;
    auto wait_last = [&]() {
      const unsigned want = epoch0 + (unsigned)depth;
      const char *fbase = uniform_ptr(&sy->flags[g][x][rg][0]);
      const unsigned poff = (unsigned)((lane % NT) * sizeof(unsigned));
      /* (a launch that gave up: its results are discarded, see ramd_dsync) */
      coop_poll(fbase, poff, want, &sy->abort, [&]() { if (lane == 0) coop_give_up(&sy->abort, host_abort, COOP_ABORT_CHAIN); });
      XC_STAMP(2);
    };
    constexpr int XQ = (K / 4 + 1 + 63) / 64; /* float4 per lane of an error row (h_size = K + 4) */
    const int r = row0 + sr;
    if constexpr (XD) /* (the operand area holds its 52 KB from hidden 512 on: launcher) */
      extras_dense_tail<512>(v, r, r - xc.row0, xc.nx, xc.nxp, xc.active, xc.flags, abuf, wait_last);
    else
      extras_control_tail<XQ, 512>(v, r, r - xc.row0, xc.nx, xc.nxp, xc.active, xc.flags, abuf, (i == j && xc_first) ? &tpre : nullptr, wait_last);
    XC_STAMP(9);
    __syncthreads();
  }
  BND_MARK(g_bnd_chain, 1);
}
