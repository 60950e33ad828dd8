// k_fwd_fused.h -- assemble + hidden layer in one launch: fwd_fused_tile and k_fwd_fused around it.
// Included by kernels_forward.hip, which launches k_fwd_fused (launch_fwd_fused_ns), and by k_fwd_top.h.
//
// The text step's forward pass shaped like a chain step (recur-nn.c:104-148): output tile =
// 32 streams x 32 hidden columns, K = the previous hidden values 1..hidden_size in 128-deep
// stages through the LDS ring, loader and compute waves of k_chain_main (the K loop: k_ring.h).  What differs:
//   * A = rows of `hidden` (the previous step's activations, K-contiguous, swizzled as in the
//     chain); B = W_ih rows k, columns of the tile: K-major, so a stage is [128 k][32 columns]
//     in LDS and a lane fetches its four k with two ds_read2_b32;
//   * the bias row (input 0 is always 1) and the row of the stream's one-hot input are added in
//     the epilogue -- the K loop never touches the input columns;
//   * the workgroup does k_assemble's work for its block on the side: it writes its 32 x 32
//     block of the new history slot (the previous hidden values), the workgroups of column tile
//     0 also the bias, the input columns, the ring index and the text target; the row sum
//     that decides the emergency soft clip (maybe_scale_inputs, recur-nn.c:68-81) falls out
//     of the A fragments, and the clip is applied to the outputs and the stored row alike;
//   * the pre-activation sums go to slab plane 0 for k_text_top (which applies the activation
//     and writes `hidden`: the A operand must stay intact while other workgroups read it); the
//     h_size padding columns, which only matter when W's padding is non-zero, come as per-tile
//     partial sums in plane 1 ([tn][nrows][4]) that k_text_top adds up.
// Launcher preconditions: every stream at the same ring position, one-hot or text input, no
// presynaptic noise, no bottom layer, hidden_size a multiple of 32.
#pragma once
#include "k_ring.h"
#include "text_pos_rule.h"

#ifdef PC_STAMPS /* development builds only (tools/mkabl.sh -DPC_STAMPS, tools/gpu_fwd_stamps.py) */
__device__ unsigned long long g_ff_stamps[8];
extern "C" void ramd_fwd_stamps(unsigned long long *out) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ff_stamps), sizeof(unsigned long long) * 8));
}
#define FF_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_ff_stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FF_STAMP(i) do { } while (0)
#endif
BND_DECL(g_bnd_fwd, ramd_bnd_fwd_stamps)
/* The work of one 32 x 32 tile (row tile mt, column tile nt) by the first eight waves of a workgroup: waves 0-3 multiply
 * and finish, waves 4-7 load.  k_fwd_fused and k_fwd_top (below) both call it, so the sums are the same bits in either.
 * NS s_barriers and one __syncthreads: waves of the workgroup that do not come here keep the count (k_fwd_top's 8-15).
 * smem: the operand ring, C_STAGES * C_STAGE_FLOATS floats of LDS; free again when the function returns.
 * MODE >= 0: the input mode as a constant (the forms of the other modes are not compiled in).
 * PARK: what the epilogue needs from memory waits in LDS, not in registers, while the K loop runs -- the same values; for
 * a caller whose waves have 128 registers (sixteen waves a workgroup), where they and the read-ahead do not fit together.
 * Five parts in a row, marked (1) .. (5): one function and not five, since each part cut out as a __forceinline__ function
 * changed the registers of k_fwd_top<8>, which has none to spare (profiles/NOTES_r19.md).  The order of the statements is
 * part of the contract (under PARK: what is derived a second time behind the K loop), and so is that of the __shared__ arrays. */
template <int NS, int MODE, bool PARK = false>
__device__ __forceinline__ void fwd_fused_tile(const View &v, float *smem, const int mt, const int nt, int new_idx, int row0,
                                               int nrows, int tn, int nstages_arg, int mode_arg, int text_i,
                                               int global_first, int n_set, const float *__restrict__ dense, int ld) {
  const int mode = MODE >= 0 ? MODE : mode_arg;
  const int nstages = NS > 0 ? NS : nstages_arg;
  __shared__ float rs_sh[4][CM];
  __shared__ float4 wt_sh[CN];
  /* dense inputs (mode RAMD_IN_DENSE: the feature vectors of gstclassify, rnnca's neighbourhoods -- up to FF_MAXIN
   * columns): the tile's 32 input rows and the W rows of the input columns under its 32 columns, for the epilogue */
  __shared__ float xin_sh[CM][FF_MAXIN + 1];
  __shared__ __attribute__((aligned(16))) float win_sh[FF_MAXIN][CN];
  __shared__ float4 wint_sh[FF_MAXIN]; /* ... and those rows' tail columns (column tile 0) */
  const RamdShape &s = v.sh;
  /* column tiles start at column 0 (16-byte aligned rows of W and of the outputs); column 0's
   * sum is never used (the bias node), and the last four columns of h_size -- hidden value
   * hidden_size and the padding -- are not in any tile: they come as partial sums */
  const int m0 = mt * CM, n0 = nt * CN;
  const int wave8 = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool loader = wave8 >= 4;
  const int wave = wave8 & 3;
  const int lm = lane & 31, kh = lane >> 5;
  const float *hid0 = v.b.hidden + (size_t)row0 * s.H;

  // --- (1) LDS-DMA sources and the issue of one stage: instruction i < 16 fills rows 2 (i & 15), +1 of A; i >= 16 fills
  // k rows 8 (i - 16) .. + 7 of B, eight lanes (32 columns) per k row
  const float *src[8];
  size_t stage_step[8];
  int kfirst[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    int i = wave * 8 + j;
    if (i < 16) {
      int row = 2 * (i & 15) + (lane >> 5);
      int c = (lane & 31) ^ (row & 15);
      int r = m0 + row;
      src[j] = hid0 + (size_t)(r < nrows ? r : nrows - 1) * s.H + 1 + 4 * c;
      stage_step[j] = CK;
      kfirst[j] = 1 + 4 * c;
    } else {
      int kr = 8 * (i - 16) + (lane >> 3);
      src[j] = v.b.ih_w + (size_t)(1 + kr) * s.H + n0 + 4 * (lane & 7);
      stage_step[j] = (size_t)CK * s.H;
      kfirst[j] = 1 + kr;
    }
  }
  auto issue = [&](int stage) {
    float *dst = smem + (stage % C_STAGES) * C_STAGE_FLOATS + wave * 8 * 256;
    const int k0 = stage * CK;
    if (k0 + CK <= s.hidden_size) {
#pragma unroll
      for (int j = 0; j < 8; j++)
        __builtin_amdgcn_global_load_lds((glb_void_t *)(src[j] + stage * stage_step[j]),
                                         (lds_void_t *)(dst + j * 256), 16, 0, 0);
      return;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) { /* last, partial stage: what lies past the hidden values is zero */
      const float *g = (k0 + kfirst[j] <= s.hidden_size) ? src[j] + stage * stage_step[j] : v.b.zeros;
      __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)(dst + j * 256), 16, 0, 0);
    }
  };

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.0f;

  /* (not const: PARK derives them a second time behind the K loop, so that they are not alive across it) */
  int etid = threadIdx.x & 255;
  int erow = etid >> 3, ec4 = (etid & 7) * 4;
  int er = m0 + erow < nrows ? m0 + erow : nrows - 1; /* row within the set */
  int grow = row0 + er;
  const int tail = s.H - 4; /* the four columns outside the tiles: hidden_size = tail or tail + 1 .. */
  if (loader) {
#pragma unroll
    for (int p = 0; p < C_STAGES - 1; p++)
      if (p < nstages) issue(p);
    /* (PARK: the loaders' whole loop here, so that their sources are not alive across the other waves' requests below --
     * the waves' own order of instructions is the same either way) */
    if constexpr (PARK) RING_LOADER_LOOP(C_STAGES, nstages, issue)
  }
  // --- (2) what the epilogue needs from memory (compute waves; PARK: kept in LDS across the K loop): the one-hot
  // index, this thread's four input
  // values x[n0 + ec4 ..] (column 0 is the bias node, 1), the bias row's and the input row's
  // weights under its four columns, and the tail columns of W in the rows of its four inputs
  int hot = -1, text_o = 0;
  float4 a4 = zero4(), wb = zero4(), ws = zero4(), wt_mine = zero4();
  /* column tile 0 also covers what no tile does (one row in eight lanes): the hidden values from `tail` on and the
   * one-hot input, times their W rows' tail columns -- requested with the rest, not in the epilogue (round 3: those
   * eight workgroups' two extra round trips were the launch's last microsecond) */
  constexpr int TAILK = 4; /* hidden values tail .. hidden_size: at most h_size - tail */
  float xt[TAILK] = {0.f, 0.f, 0.f, 0.f};
  float4 wtl[TAILK] = {zero4(), zero4(), zero4(), zero4()}, wth = zero4();
  bool tail_row = nt == 0 && (etid & 7) == 0;
  const bool dns = mode == RAMD_IN_DENSE;
  const int insz = dns ? s.input_size : 0;
  float xin_r[CM * FF_MAXIN / 256]; /* requested here, stored to LDS behind the K loop: nobody waits for them */
  float4 win_r[FF_MAXIN * (CN / 4) / 256], wint_r = zero4();
  if (!loader && dns) {
#pragma unroll
    for (int u = 0; u < CM * FF_MAXIN / 256; u++) {
      const int idx = etid + 256 * u, rr = idx / insz, k = idx - rr * insz;
      const int rc = m0 + rr < nrows ? m0 + rr : nrows - 1;
      xin_r[u] = idx < CM * insz ? dense[(size_t)rc * ld + k] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < FF_MAXIN * (CN / 4) / 256; u++) {
      const int idx = etid + 256 * u, k = idx >> 3;
      win_r[u] = k < insz ? ld4(v.b.ih_w + (size_t)(s.hidden_size + 1 + k) * s.H + n0 + 4 * (idx & 7)) : zero4();
    }
    if (nt == 0 && etid < insz) wint_r = ld4(v.b.ih_w + (size_t)(s.hidden_size + 1 + etid) * s.H + tail);
  }
  if (!loader) {
    if (mode == RAMD_IN_TEXT) {
      text_o = text_pos(v.b.text_len, n_set, global_first + er, text_i);
      hot = v.b.text[text_o];
    } else if (!dns) {
      hot = v.b.hot[grow];
    }
    a4 = ld4(hid0 + (size_t)er * s.H + n0 + ec4);
    wb = ld4(v.b.ih_w + n0 + ec4);
    /* the tail columns of W in this tile's 32 input rows: one row per thread of the first half
     * wave, shared through LDS at the end */
    if (etid < CN) wt_mine = ld4(v.b.ih_w + (size_t)(n0 + etid) * s.H + tail);
    if (tail_row) {
#pragma unroll
      for (int i = 0; i < TAILK; i++) {
        const int k = tail + i <= s.hidden_size ? tail + i : tail;
        xt[i] = hid0[(size_t)er * s.H + k];
        wtl[i] = ld4(v.b.ih_w + (size_t)k * s.H + tail);
      }
    }
  }
  if (!loader) { /* ... and what depends on the symbol (a load behind a load) */
    if (hot < 0 || hot >= s.input_size) hot = -1;
    if (n0 + ec4 == 0) a4.x = 1.0f;
    ws = ld4(v.b.ih_w + (size_t)(hot >= 0 ? s.hidden_size + 1 + hot : 0) * s.H + n0 + ec4);
    if (tail_row) wth = ld4(v.b.ih_w + (size_t)(hot >= 0 ? s.hidden_size + 1 + hot : 0) * s.H + tail);
  }
  /* PARK: they go to LDS as they land (the ones behind one load about when the first operand stage does, the two behind
   * the symbol's load a round trip later) */
  __shared__ float4 park_sh[PARK ? 3 : 1][PARK ? 256 : 1];
  __shared__ float4 park_tail_sh[PARK ? TAILK + 2 : 1][PARK ? CM : 1];
  __shared__ int park_sym_sh[PARK ? 2 : 1][PARK ? 256 : 1];
  if constexpr (PARK) {
    if (!loader) {
      park_sh[0][etid] = a4;
      park_sh[1][etid] = wb;
      park_sh[2][etid] = ws;
      park_sym_sh[0][etid] = hot;
      park_sym_sh[1][etid] = text_o;
      if (etid < CN) wt_sh[etid] = wt_mine;
      if (tail_row) {
        park_tail_sh[TAILK][erow] = make_float4(xt[0], xt[1], xt[2], xt[3]);
        park_tail_sh[TAILK + 1][erow] = wth;
#pragma unroll
        for (int i = 0; i < TAILK; i++) park_tail_sh[i][erow] = wtl[i];
      }
    }
  }
  // --- (3) the K loop (k_ring.h)
  const uint32_t lds0 = lds_byte_addr(smem);
  const uint32_t rowoff = (uint32_t)lm * (CK * 4u);
  float rsum = 0.0f;
  if (loader) {
    if constexpr (!PARK) RING_LOADER_LOOP(C_STAGES, nstages, issue)
  } else {
    struct Frag { f32x4 a[4]; f32x2 lo[4], hi[4]; };
    auto rd = [&](int st, Frag &f) {
      if (st == 0) FF_STAMP(2); /* (development builds: the first stage has landed) */
      const uint32_t abase = lds0 + (uint32_t)((st % C_STAGES) * C_STAGE_FLOATS) * 4u;
      const uint32_t bbase = abase + (uint32_t)(CM * CK) * 4u;
#pragma unroll
      for (int gi = 0; gi < 4; gi++) {
        int c = 2 * (4 * wave + gi) + kh; /* chunk = 4 consecutive k */
        f.a[gi] = lds_read_b128(abase + rowoff + (uint32_t)((c ^ (lm & 15)) * 16));
        const uint32_t baddr = bbase + (uint32_t)((4 * c) * CN + lm) * 4u;
        f.lo[gi] = lds_read2_b32(baddr);
        f.hi[gi] = lds_read2_b32_hi(baddr);
      }
    };
    auto multiply = [&](const Frag &f) {
#pragma unroll
      for (int gi = 0; gi < 4; gi++) {
        mfma_k4(acc, f.a[gi], f.lo[gi].x, f.lo[gi].y, f.hi[gi].x, f.hi[gi].y);
        rsum += (f.a[gi].x + f.a[gi].y) + (f.a[gi].z + f.a[gi].w);
      }
    };
    auto step = [&](int st, Frag &f, Frag &fn) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (st + 1 < nstages) {
        __builtin_amdgcn_s_barrier();
        rd(st + 1, fn);
      }
      __builtin_amdgcn_sched_barrier(0);
      multiply(f);
      __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (NS > 0) {
      FF_STAMP(1);
      RING_READ_AHEAD(NS, Frag, rd, step)
    } else { /* any number of stages: no read-ahead (k_ring.h says why) */
      Frag f;
      for (int st = 0; st < nstages; st++) {
        __builtin_amdgcn_s_barrier();
        rd(st, f);
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.lo[0]), "+v"(f.lo[1]),
                       "+v"(f.lo[2]), "+v"(f.lo[3]), "+v"(f.hi[0]), "+v"(f.hi[1]), "+v"(f.hi[2]), "+v"(f.hi[3])
                     :
                     : "memory");
        multiply(f);
      }
    }
  }
  // --- (4) the four waves' tiles and row sums through LDS
  float *red = smem + (nstages % C_STAGES) * C_STAGE_FLOATS; /* [4][32][32] */
  if (!loader) FF_STAMP(3);
  if (!loader) {
#pragma unroll
    for (int g = 0; g < 16; g++) {
      int row = (g & 3) + 8 * (g >> 2) + 4 * kh;
      red[(wave * CM + row) * CN + lm] = acc[g];
    }
    rsum += __shfl_xor(rsum, 32, 64);
    if (kh == 0) rs_sh[wave][lm] = rsum;
    if (!PARK && etid < CN) wt_sh[etid] = wt_mine;
    if (dns) {
#pragma unroll
      for (int u = 0; u < CM * FF_MAXIN / 256; u++) {
        const int idx = etid + 256 * u, rr = idx / insz, k = idx - rr * insz;
        if (idx < CM * insz) xin_sh[rr][k] = xin_r[u];
      }
#pragma unroll
      for (int u = 0; u < FF_MAXIN * (CN / 4) / 256; u++) {
        const int idx = etid + 256 * u, k = idx >> 3;
        if (k < insz) *reinterpret_cast<float4 *>(&win_sh[k][4 * (idx & 7)]) = win_r[u];
      }
      if (nt == 0 && etid < insz) wint_sh[etid] = wint_r;
    }
  }
  __syncthreads();
  if (loader) return;
  FF_STAMP(4);
  if constexpr (PARK) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid)); /* (the compiler is not to know that these are the values it had before the loop) */
    etid = tid & 255;
    erow = etid >> 3, ec4 = (etid & 7) * 4;
    er = m0 + erow < nrows ? m0 + erow : nrows - 1;
    grow = row0 + er;
    tail_row = nt == 0 && (etid & 7) == 0;
    hot = park_sym_sh[0][etid];
    text_o = park_sym_sh[1][etid];
    a4 = park_sh[0][etid];
    wb = park_sh[1][etid];
    ws = park_sh[2][etid];
    { /* (every lane, not the tail rows' alone: a lane that kept its old values would keep them alive across the loop;
       * what the others read is never used) */
      wth = park_tail_sh[TAILK + 1][erow];
      const float4 x4 = park_tail_sh[TAILK][erow];
      xt[0] = x4.x, xt[1] = x4.y, xt[2] = x4.z, xt[3] = x4.w;
#pragma unroll
      for (int i = 0; i < TAILK; i++) wtl[i] = park_tail_sh[i][erow];
    }
  }
  // --- (5) the epilogue: soft clip, the block's stores, the tail columns' partial sums, the rest of k_assemble's row
  const int row = erow, c4 = ec4;
  float4 wt[4];
#pragma unroll
  for (int i = 0; i < 4; i++) wt[i] = wt_sh[c4 + i];
  float4 e;
  {
    float4 p0 = ld4(red + (0 * CM + row) * CN + c4), p1 = ld4(red + (1 * CM + row) * CN + c4);
    float4 p2 = ld4(red + (2 * CM + row) * CN + c4), p3 = ld4(red + (3 * CM + row) * CN + c4);
    e.x = (p0.x + p1.x) + (p2.x + p3.x);
    e.y = (p0.y + p1.y) + (p2.y + p3.y);
    e.z = (p0.z + p1.z) + (p2.z + p3.z);
    e.w = (p0.w + p1.w) + (p2.w + p3.w);
  }
  // dense inputs: their products under this thread's four columns (the input rows of W_ih lie behind the hidden
  // values', recur-nn.c:104-112), and their sum
  float4 din = zero4();
  float sum_in = 0.0f;
  for (int k = 0; k < insz; k++) {
    const float x = xin_sh[row][k];
    const float4 w = *reinterpret_cast<const float4 *>(&win_sh[k][c4]);
    din.x += x * w.x; din.y += x * w.y; din.z += x * w.z; din.w += x * w.w;
    sum_in += x;
  }
  // the row's input sum: bias + previous hidden values + the one-hot input (or the dense ones)
  float sum = ((rs_sh[0][row] + rs_sh[1][row]) + (rs_sh[2][row] + rs_sh[3][row])) + 1.0f +
              (dns ? sum_in : hot >= 0 ? 1.0f : 0.0f);
  const float softclip = s.I * INPUT_MEAN_SOFT_TOP_F;
  const float scale = (sum > softclip) ? soft_clip_dev(sum, softclip) : 1.0f;
  const bool live = m0 + row < nrows;
  // this workgroup's share of the four tail columns: its 32 inputs x W[k][tail .. tail + 3]
  float4 pp;
  pp.x = ((a4.x * wt[0].x + a4.y * wt[1].x) + (a4.z * wt[2].x + a4.w * wt[3].x));
  pp.y = ((a4.x * wt[0].y + a4.y * wt[1].y) + (a4.z * wt[2].y + a4.w * wt[3].y));
  pp.z = ((a4.x * wt[0].z + a4.y * wt[1].z) + (a4.z * wt[2].z + a4.w * wt[3].z));
  pp.w = ((a4.x * wt[0].w + a4.y * wt[1].w) + (a4.z * wt[2].w + a4.w * wt[3].w));
  /* the eight lanes of a row: two quad permutes and a half-row mirror (DPP: a few cycles each; as __shfl_xor twelve
   * dependent ds_bpermute round trips in the launch's last microsecond) */
#define FF_DPP_ADD(x, ctrl) x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), ctrl, 0xf, 0xf, true))
  FF_DPP_ADD(pp.x, 0xB1); FF_DPP_ADD(pp.y, 0xB1); FF_DPP_ADD(pp.z, 0xB1); FF_DPP_ADD(pp.w, 0xB1);
  FF_DPP_ADD(pp.x, 0x4E); FF_DPP_ADD(pp.y, 0x4E); FF_DPP_ADD(pp.z, 0x4E); FF_DPP_ADD(pp.w, 0x4E);
  FF_DPP_ADD(pp.x, 0x141); FF_DPP_ADD(pp.y, 0x141); FF_DPP_ADD(pp.z, 0x141); FF_DPP_ADD(pp.w, 0x141);
#undef FF_DPP_ADD
  if (!live) return;
  float *out = v.b.slab + (size_t)er * s.H;
  float *slot = v.b.arena + ((size_t)new_idx * s.Scap + grow) * s.I;
  {
    float4 o;
    o.x = ((e.x + wb.x) + (dns ? din.x : hot >= 0 ? ws.x : 0.0f)) * scale;
    o.y = ((e.y + wb.y) + (dns ? din.y : hot >= 0 ? ws.y : 0.0f)) * scale;
    o.z = ((e.z + wb.z) + (dns ? din.z : hot >= 0 ? ws.z : 0.0f)) * scale;
    o.w = ((e.w + wb.w) + (dns ? din.w : hot >= 0 ? ws.w : 0.0f)) * scale;
    *reinterpret_cast<float4 *>(out + n0 + c4) = o;
    *reinterpret_cast<float4 *>(slot + n0 + c4) = make_float4(a4.x * scale, a4.y * scale, a4.z * scale, a4.w * scale);
  }
  if ((etid & 7) == 0) {
    if (nt == 0) {
      /* once per row: the inputs the tiles do not cover -- hidden values tail .. hidden_size and
       * the one-hot input -- times their W rows */
#pragma unroll
      for (int i = 0; i < TAILK; i++) {
        if (tail + i <= s.hidden_size) {
          const float x = xt[i];
          const float4 w = wtl[i];
          pp.x += x * w.x; pp.y += x * w.y; pp.z += x * w.z; pp.w += x * w.w;
          slot[tail + i] = x * scale;
        }
      }
      if (hot >= 0) {
        pp.x += wth.x; pp.y += wth.y; pp.z += wth.z; pp.w += wth.w;
      }
      for (int k = 0; k < insz; k++) {
        const float x = xin_sh[row][k];
        const float4 w = wint_sh[k];
        pp.x += x * w.x; pp.y += x * w.y; pp.z += x * w.z; pp.w += x * w.w;
      }
    }
    float *pd = v.b.slab + (size_t)nrows * s.H + ((size_t)nt * nrows + er) * 4;
    *reinterpret_cast<float4 *>(pd) = make_float4(pp.x * scale, pp.y * scale, pp.z * scale, pp.w * scale);
  }
  /* (by column tile 1's workgroups where there is one: column tile 0's have the tail columns' extra loads and sums above,
   * and were the launch's last to end by 0.9 us -- round 6, the workgroups' own marks) */
  if (nt == (tn > 1 ? 1 : 0)) { /* the rest of k_assemble's row: input columns, ring index, target */
    const int sub = etid & 7;
    if (sub == 0) {
      v.b.idx[grow] = new_idx;
      if (mode == RAMD_IN_TEXT) v.b.target[grow] = v.b.text[text_o + 1];
    }
    if (dns)
      for (int k = sub; k < s.input_size; k += 8) slot[s.hidden_size + 1 + k] = xin_sh[row][k] * scale;
    else
      for (int k = sub; k < s.input_size; k += 8) slot[s.hidden_size + 1 + k] = (k == hot) ? scale : 0.0f;
  }
  FF_STAMP(5);
}

template <int NS = 0>
__global__ __launch_bounds__(512) void k_fwd_fused(const View *__restrict__ vp, int new_idx, int row0, int nrows, int tm, int tn,
                                                   int nstages_arg, int mode, int text_i, int global_first, int n_set,
                                                   const float *__restrict__ dense, int ld) {
  FF_STAMP(0);
  BND_MARK(g_bnd_fwd, 0);
  View v = *vp;
  __shared__ __attribute__((aligned(16))) float smem[C_STAGES * C_STAGE_FLOATS];
  const int L = blockIdx.x;
  const int xcd = L & 7, q = L >> 3;
  const int mt = q % tm, nt = (q / tm) * 8 + xcd;
  if (nt >= tn) return;
  fwd_fused_tile<NS, -1>(v, smem, mt, nt, new_idx, row0, nrows, tn, nstages_arg, mode, text_i, global_first, n_set, dense, ld);
  BND_MARK(g_bnd_fwd, 1);
}
