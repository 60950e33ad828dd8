// k_fwd_stages.h -- the element-wise stages of the forward pass around the hidden-layer GEMM: the ring advance, input
// assembly, the bottom layer, the presynaptic noise in its three kernels, the two finishing kernels and the plain sum of
// K slabs.  Included by kernels_forward.hip, which launches them (stage_input, stage_noise, stage_hidden_end).
#pragma once
#include "k_common.h"
#include "text_pos_rule.h"

// rnn_bptt_advance (recur-nn.c:696-704) for a range of training streams
__global__ void k_advance(View v, int row0, int nrows) {
  int r = row0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (r < row0 + nrows && r < v.sh.Scap) {
    int i = v.b.idx[r] + 1;
    if (i == v.sh.D) i -= v.sh.D;
    v.b.idx[r] = i;
  }
}

// Builds the input row of each stream: previous hiddens, bias, real inputs
// (recur-nn.c:104-112) and the emergency soft clip of the whole row
// (maybe_scale_inputs, recur-nn.c:68-81).  One workgroup per stream.
__global__ __launch_bounds__(256) void k_assemble(View v, int row0, int mode, const float *dense, int ld, int text_i,
                                                  int global_first, int n_set, int advance) {
  __shared__ float red[4];
  const RamdShape &s = v.sh;
  int j = blockIdx.x;
  int r = row0 + j;
  float *slot;
  if (r < s.Scap) {
    int i = v.b.idx[r];
    if (advance) { /* rnn_bptt_advance (recur-nn.c:696-704) for this stream, done here */
      i = (i + 1 == s.D) ? 0 : i + 1;
      __syncthreads(); /* every thread has read the old index */
      if (threadIdx.x == 0) v.b.idx[r] = i;
    }
    slot = v.b.arena + ((size_t)i * s.Scap + r) * s.I;
  } else {
    slot = input_row(v, r, 0);
  }
  const float *hid = v.b.hidden + (size_t)r * s.H;
  int hot = -1;
  if (mode == RAMD_IN_ONE_HOT) {
    hot = v.b.hot[r];
  } else if (mode == RAMD_IN_TEXT) {
    const int o = text_pos(v.b.text_len, n_set, global_first + j, text_i);
    hot = v.b.text[o];
    if (threadIdx.x == 0) v.b.target[r] = v.b.text[o + 1];
  }
  assemble_input_row(s, slot, hid, mode, hot, mode == RAMD_IN_DENSE ? dense + (size_t)j * ld : nullptr, red);
}

// plain "sum the K slabs" finalize: dst[r][c] (+)= sum_z slab[z][r][c]
__global__ __launch_bounds__(256) void k_sum_slabs(float *dst, int ld_dst, const float *slab, int M, int N, int ks, int accumulate) {
  int q = blockIdx.x * 256 + threadIdx.x;
  int per_row = N >> 2;
  if (q >= M * per_row) return;
  int r = q / per_row, c = (q - r * per_row) * 4;
  const float *p = slab + (size_t)r * N + c;
  float4 a = accumulate ? ld4(dst + (size_t)r * ld_dst + c) : zero4();
  for (int z = 0; z < ks; z++) add4(a, ld4(p + (size_t)z * M * N));
  *reinterpret_cast<float4 *>(dst + (size_t)r * ld_dst + c) = a;
}

/* Sixteen values of a stream's noise row from its generator, for columns i0 .. i0 + 15 of H: column 0 gets none
 * (recur-nn.c:120-121: i from 1), the pad columns up to H do, columns past H none.  Both generating
 * kernels ask here, so the values generated ahead are the bits of the ones generated in place. */
__device__ __forceinline__ void noise_piece16(DevRng &g, int i0, int H, float deviation, float (&nz)[16]) {
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int i = i0 + k;
    nz[k] = (i >= 1 && i < H) ? dev_cheap_gaussian(g) * deviation : 0.0f;
  }
}

// MAYBE_ADD_ARRAY_NOISE on hidden[1..h_size) (recur-nn.c:120-121).  The generator is sequential per stream, so one thread
// walks each stream's row; the values are added to K slab 0 of the forward GEMM.
/* One lane per stream: the stream's generator is a sequential recurrence (three rand64 per
 * value).  The row is walked in pieces of 16 values whose old contents are requested BEFORE the
 * piece's 48 generator steps and added and stored after them, so the memory round trips sit in
 * the shadow of the recurrence (element by element, as a read-modify-write per value, this kernel
 * took 360 us for 256 streams of 1028 values). */
__global__ void k_presynaptic_noise(View v, int row0, int nrows, float deviation) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nrows) return;
  const RamdShape &s = v.sh;
  DevRng g = reinterpret_cast<DevRng *>(v.b.rng)[row0 + j];
  float *row = v.b.slab + (size_t)j * s.H;
  for (int i0 = 0; i0 < s.H; i0 += 16) { /* h_size is a multiple of 4 */
    const int n4 = min(4, (s.H - i0) / 4);
    float4 old[4];
#pragma unroll
    for (int k = 0; k < 4; k++) old[k] = k < n4 ? ld4(row + i0 + 4 * k) : zero4();
    float nz[16];
    noise_piece16(g, i0, s.H, deviation, nz);
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < n4)
        *reinterpret_cast<float4 *>(row + i0 + 4 * k) =
            make_float4(old[k].x + nz[4 * k], old[k].y + nz[4 * k + 1], old[k].z + nz[4 * k + 2], old[k].w + nz[4 * k + 3]);
  }
  reinterpret_cast<DevRng *>(v.b.rng)[row0 + j] = g;
}

/* The same values without touching anything: out[j][1..H) and the generator state after them
 * (noise_ahead.c: runs on a second stream while the rest of the previous generation is still being
 * computed; noise_ahead.h says when a pass may take them) */
/* src / tclass / skip: the forms for the multi-head step -- start from the states an earlier pass left (`src`: the ones
 * the pass before adopted, or the ones the speculation before this one wrote) and first make the draws the multi-head
 * loss makes from the stream's generator in between, one per head other than the stream's own
 * (k_multi_softmax_error): `ncls` heads with the classes in `tclass`, or `skip` draws for every stream where the classes
 * are not known yet -- so that the values are those of the pass AFTER that loss although the loss has not run */
__global__ void k_noise_speculate(View v, int row0, int nrows, float deviation, float *out, DevRng *state,
                                  const DevRng *src, const int *tclass, int ncls, int skip) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nrows) return;
  const RamdShape &s = v.sh;
  DevRng g = src ? src[j] : reinterpret_cast<DevRng *>(v.b.rng)[row0 + j];
  if (tclass) {
    const int own = tclass[j];
    skip = ncls - ((own >= 0 && own < ncls) ? 1 : 0);
  }
  for (int i = 0; i < skip; i++) (void)dev_rand64(g);
  float *row = out + (size_t)j * s.H;
  for (int i0 = 0; i0 < s.H; i0 += 16) {
    float nz[16];
    noise_piece16(g, i0, s.H, deviation, nz);
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (i0 + 4 * k < s.H)
        *reinterpret_cast<float4 *>(row + i0 + 4 * k) = make_float4(nz[4 * k], nz[4 * k + 1], nz[4 * k + 2], nz[4 * k + 3]);
  }
  state[j] = g;
}
/* (Round 6, measured and removed: a WAVE per stream with the recurrence on the scalar unit -- four 64-bit scalar
 * registers, s_lshl_b64 / s_or_b64 / s_add_u32 + s_addc_u32, the twelve 16-bit fields of a value added two at a time in
 * the halves of a 64-bit word, lane k keeping value k of 64: bit-exact, and SLOWER -- 283 against 218 us per generation
 * of 32 streams, 384 against 338 of 256: a dependent scalar instruction takes ~7 cycles here, and the form has 85 of them
 * per value against the vector form's 60.  profiles/NOTES_r06.md.) */

/* ... and their use by the forward pass, in two halves (k_noise_apply stores its sums between them): the values ... */
__device__ __forceinline__ float4 noise_ahead4(const View &v, int j, int c) {
  return ld4(v.b.noise_spec + (size_t)j * v.sh.H + c);
}
/* ... and, by the thread that has column 0, the generator of the stream (state row row0 + j) = the state after them */
__device__ __forceinline__ void adopt_noise_state(const View &v, int row0, int j, int c) {
  if (c == 0) reinterpret_cast<DevRng *>(v.b.rng)[row0 + j] = reinterpret_cast<const DevRng *>(v.b.rng_spec)[j];
}
/* slab plane 0 += values, generators = the states after them */
__global__ __launch_bounds__(256) void k_noise_apply(View v, int row0, int nrows) {
  const RamdShape &s = v.sh;
  const int q = blockIdx.x * 256 + threadIdx.x, per_row = s.H >> 2;
  if (q >= nrows * per_row) return;
  const int j = q / per_row, c = (q - j * per_row) * 4;
  float4 a = ld4(v.b.slab + (size_t)j * s.H + c);
  add4(a, noise_ahead4(v, j, c));
  *reinterpret_cast<float4 *>(v.b.slab + (size_t)j * s.H + c) = a;
  adopt_noise_state(v, row0, j, c);
}

// The optional bottom layer of rnn_opinion (recur-nn.c:88-103): one workgroup per
// stream.  The layer is small (tens to a few hundred nodes each side), so each output
// column is one thread's sequential dot product down the rows, in the reference's
// order (calculate_interlayer, recur-nn.c:18-65, skips zero inputs).  The noise comes
// from the stream's own generator before the hidden layer draws from it.
__global__ __launch_bounds__(256) void k_bottom_forward(View v, int row0, int mode, const float *dense, int ld, int text_i,
                                                        int global_first, int n_set, float deviation) {
  extern __shared__ float bsh[];
  const RamdShape &s = v.sh;
  float *sin = bsh, *sout = bsh + s.bI;
  int j = blockIdx.x;
  int r = row0 + j;
  float *inp = v.b.binp + (size_t)r * s.bI;
  int hot = -1;
  if (mode == RAMD_IN_ONE_HOT) {
    hot = v.b.hot[r];
  } else if (mode == RAMD_IN_TEXT) {
    const int o = text_pos(v.b.text_len, n_set, global_first + j, text_i);
    hot = v.b.text[o];
    if (threadIdx.x == 0) v.b.target[r] = v.b.text[o + 1];
  }
  for (int i = threadIdx.x; i < s.bI; i += 256) {
    float x;
    if (i == 0) x = 1.0f;
    else if (i > s.b_in || mode == RAMD_IN_KEEP) x = inp[i];
    else if (mode == RAMD_IN_DENSE) x = dense[(size_t)j * ld + (i - 1)];
    /* one_hot_opinion's bottom-layer branch clears and indexes the layer's inputs from
     * the bias slot (charmodel-helpers.h:20-23, 30-31): symbol k lights entry k, the
     * last entry is never cleared */
    else if (i == s.b_in) x = v.b.blast[0]; /* ONE buffer for all clones: what the last dense pass of ANY stream left */
    else x = (i == hot) ? 1.0f : 0.0f;
    inp[i] = x;
    sin[i] = x;
    if (i == s.b_in && (mode == RAMD_IN_DENSE || mode == RAMD_IN_KEEP) && j == (int)gridDim.x - 1)
      v.b.blast[0] = x; /* the last stream of the pass is the one whose inputs stay in the buffer */
  }
  __syncthreads();
  for (int x = threadIdx.x; x < s.bO; x += 256) {
    float acc = 0.0f;
    for (int y = 0; y < s.bI; y++) {
      float xi = sin[y];
      if (xi != 0.0f) acc += xi * v.b.bw[y * s.bO + x];
    }
    sout[x] = acc;
  }
  __syncthreads();
  if (deviation != 0.0f && threadIdx.x == 0) {
    DevRng g = reinterpret_cast<DevRng *>(v.b.rng)[r];
    for (int i = 1; i < s.input_size; i++) sout[i] += dev_cheap_gaussian(g) * deviation;
    reinterpret_cast<DevRng *>(v.b.rng)[r] = g;
  }
  __syncthreads();
  float *slot = input_row<false>(v, r, 0) + s.hidden_size + 1;
  float *out = v.b.bout + (size_t)r * s.bO;
  for (int x = threadIdx.x; x < s.bO; x += 256) {
    float o = sout[x];
    out[x] = o;
    if (x < s.input_size) slot[x] = o > 0.0f ? o : 0.0f;
  }
}

/* The end of both finishing kernels, for the four sums `a` of stream j from column c on: the activation
 * (recur-nn.c:123-148), the bias node at column 0 and the store into `hidden`. */
__device__ __forceinline__ void finish_hidden4(const View &v, int row0, int j, int c, const float4 &a) {
  float h[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
  for (int i = 0; i < 4; i++) h[i] = act_forward(v.sh, h[i]);
  if (c == 0) h[0] = 1.0f; /* the bias node, recur-nn.c:148 */
  *reinterpret_cast<float4 *>(v.b.hidden + (size_t)(row0 + j) * v.sh.H + c) = make_float4(h[0], h[1], h[2], h[3]);
}

// sums the K slabs, applies the activation and writes the hidden rows.  Element-wise, float4 per thread.
__global__ __launch_bounds__(256) void k_fwd_finalize(View v, int row0, int nrows, int ks) {
  const RamdShape &s = v.sh;
  int q = blockIdx.x * 256 + threadIdx.x; /* float4 index */
  int per_row = s.H >> 2;
  if (q >= nrows * per_row) return;
  int j = q / per_row, c = (q - j * per_row) * 4;
  const float *p = v.b.slab + (size_t)j * s.H + c;
  /* (its own plane sum, from plane 0 on: k_common.h's sum_planes adds onto a zero first, other bits for a -0.0f sum) */
  float4 a = ld4(p);
  for (int z = 1; z < ks; z++) add4(a, ld4(p + (size_t)z * nrows * s.H));
  finish_hidden4(v, row0, j, c, a);
}

// the same for k_fwd_fused's result (one plane of sums for the columns inside its tiles, per-tile partial sums
// [tn][nrows][4] for the last four columns of h_size): the set calls that go on to a generic output layer, where
// k_text_top is not there to do it.  with_spec: the presynaptic noise generated ahead (noise_ahead.c) is added here
// and its generator states adopted (k_noise_apply's work).
__global__ __launch_bounds__(256) void k_fwd_finalize_fused(View v, int row0, int nrows, int tn, int with_spec, int nmain) {
  const RamdShape &s = v.sh;
  const int per_row = (s.H >> 2) - 1; /* float4s of a row inside the tiles */
  int j, c;
  float4 a;
  if ((int)blockIdx.x < nmain) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nrows * per_row) return;
    j = q / per_row;
    c = (q - j * per_row) * 4;
    a = ld4(v.b.slab + (size_t)j * s.H + c);
  } else {
    /* the last four columns: 32 lanes per row, lane t the partial sums of tiles t, t + 32, ..; eight rows per workgroup */
    const int t = threadIdx.x & 31;
    j = ((int)blockIdx.x - nmain) * 8 + (threadIdx.x >> 5);
    c = s.H - 4;
    const int jc = min(j, nrows - 1);
    a = zero4();
    for (int tt = t; tt < tn; tt += 32) add4(a, ld4(v.b.slab + (size_t)nrows * s.H + ((size_t)tt * nrows + jc) * 4));
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
      a.x += __shfl_xor(a.x, off, 64);
      a.y += __shfl_xor(a.y, off, 64);
      a.z += __shfl_xor(a.z, off, 64);
      a.w += __shfl_xor(a.w, off, 64);
    }
    if (t != 0 || j >= nrows) return;
  }
  if (with_spec) {
    add4(a, noise_ahead4(v, j, c));
    adopt_noise_state(v, row0, j, c);
  }
  finish_hidden4(v, row0, j, c, a);
}
