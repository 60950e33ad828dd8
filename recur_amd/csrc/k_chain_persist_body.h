// k_chain_persist_body.h -- the body of k_chain_persist and of k_chain_persist_early (k_chain_persist.h includes it inside
// each of the two kernels, which differ in EARLY alone: two kernels of one text, because a body shared through a device
// function changed the instructions of the instantiations that exist).  It expects ACT, K, ONE, PAD, XD and EARLY as
// compile-time constants and the kernels' arguments by their names.
// (No include guard: it is meant to be included twice.  The names it needs, checked here so that a third includer learns
// of them from one message and not from four hundred.)
static_assert((ACT == 1 || ACT == 2 || ACT == 5) && (K == 1024 || K == 512 || K == 256) && EARLY >= 0 && EARLY < K / 64 &&
                  (ONE || !ONE) && (PAD || !PAD) && (XD || !XD) && (EARLY == 0 || (!ONE && !PAD)),
              "k_chain_persist_body.h is included inside a kernel that has ACT, K, ONE, PAD, XD and EARLY as compile-time constants");
static_assert(sizeof(vp) + sizeof(uniform_idx) + sizeof(row0) + sizeof(nrows) + sizeof(depth) + sizeof(seq) + sizeof(sy) +
                      sizeof(host_abort) + sizeof(nvalid) + sizeof(vlo) + sizeof(hw) + sizeof(xc) + sizeof(static_map) +
                      sizeof(tseq) + sizeof(seats) > 0,
              "... and k_chain_persist's fifteen arguments by these names");
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
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      /* K block u of the burst: 8 MFMAs on the fragments requested three blocks ago, the request for block u + 3 */
      auto block = [&](auto UC) {
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
        if (!ONE && (((K == 1024 ? (EARLY > 0 ? PC_GAPS_EARLY : PC_GAPS) : K == 512 ? PC_GAPS_512 : PC_GAPS_256) >> u) & 1)) { /* (ONE: nobody polls beside a burst) */
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_sleep(1);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
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
         * wave that issues f32 MFMAs back to back a store's acknowledgement comes 1-4 us late.
         * Round 20: ONE K block of the wave's own next burst in this window (EARLY, below) is the exception: 8 MFMAs,
         * 256 cycles, delay the flag by 0.03 us and take 0.10 us off the burst behind it (stamps: k_chain_persist.h, at
         * PC_GAPS_EARLY) -- 2 us and more per generation once the pauses and the first poll are retuned to it
         * (profiles/NOTES_r20.md); with two blocks every mask tried was slower than with one. */
        if constexpr (EARLY == 0) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) g_store_saddr(0u, __uint_as_float(epoch0 + (unsigned)t + 1u), &sy->flags[g][xf][wv][j]);
          PC_STAMP(0, k, 3);
        }
      }
      if constexpr (EARLY > 0) {
        /* Round 20: the burst's first EARLY blocks while the row stores are on their way -- the wave's OWN next MFMAs,
         * which need nothing the drain waits for (fenced: hipcc is free to move an MFMA across an asm wait).  Nothing
         * but the blocks stands here: the loop's counted lgkmcnt waits see the queue they always saw.  The flag stays
         * behind the drain -- in front of it the consumers would fetch rows that have not arrived -- and the gate
         * loads stay behind the flag: in front of it the drain would wait for them too.  (The first half-step has no
         * finish and nothing to drain; its blocks stand here as well, so that the burst exists once.) */
        if (multiplies) {
          __builtin_amdgcn_sched_barrier(0);
          static_for<EARLY>(block);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (k >= 1) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) g_store_saddr(0u, __uint_as_float(epoch0 + (unsigned)((k - 1) >> 1) + 1u), &sy->flags[g][xf][wv][j]);
          PC_STAMP(0, k, 3);
        }
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
      static_for<KB - EARLY>([&](auto UC) { block(std::integral_constant<int, EARLY + decltype(UC)::value>{}); });
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
    if constexpr (EARLY > 0) {
      /* (hipcc peels the first pair off this form's loop otherwise: the burst four times in the code instead of twice) */
#pragma clang loop unroll(disable)
      for (int k = 0;; k += 2) {
        if (!half(std::integral_constant<int, 0>{}, k)) break;
        if (!half(std::integral_constant<int, 1>{}, k + 1)) break;
      }
    } else {
      for (int k = 0;; k += 2) {
        if (!half(std::integral_constant<int, 0>{}, k)) break;
        if (!half(std::integral_constant<int, 1>{}, k + 1)) break;
      }
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
    __builtin_amdgcn_s_sleep(ONE ? PC_SLEEP0_ONE : K == 1024 ? (EARLY > 0 ? PC_SLEEP0_EARLY : PC_SLEEP0) : PC_SLEEP0_SMALL);
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
