// k_fwd_small.h -- one stream of a small net: the whole forward pass as one workgroup.  Included by kernels_forward.hip,
// which launches it (stage_hidden).
#pragma once
#include "k_common.h"
// ------------------------------------ one stream, small net: forward in one launch --
//
// rnn_opinion for ONE stream of a small net (recur-nn.c:83-154 without noise and bottom layer):
// the input row (bias, previous hidden values, the inputs the caller put there, the emergency
// soft clip of maybe_scale_inputs), hidden = act(x . W_ih) with the zero-row skip, bias node,
// out = hidden . W_ho -- k_assemble + k_gemm + k_fwd_finalize + k_out_layer as one workgroup.
// Thread (g = tid / HC, n = tid % HC) walks the input rows y = g, g + G, .. of column n (a wave
// reads whole contiguous rows of W_ih), the G partial sums per column are added in order.
// Preconditions (launcher): h_size <= 256, i_size <= 512, o_size <= 64.
__global__ __launch_bounds__(1024) void k_fwd_small(View v, int r) {
  __shared__ float xs[512], hsh[256], part[1024], red[16];
  const RamdShape &s = v.sh;
  const int I = s.I, H = s.H, O = s.O, hs = s.hidden_size;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  /* Round 6: this thread's weights of BOTH layers are requested before anything else -- they depend on nothing the launch
   * computes (the ring index, the input row and the hidden row were dependent round trips in front of them: 9.2 -> 8.2 us
   * per launch).  A row whose input is zero is skipped as before (a select on the input value: the weight is not
   * multiplied). */
  constexpr int FS_WI = 32, FS_WO = 16; /* rows per thread at most */
  const int HCp = H <= 128 ? 128 : 256, Gp = 1024 / HCp;
  const int np = tid & (HCp - 1), gp = tid / HCp;
  const bool pre_ok = (I + Gp - 1) / Gp <= FS_WI && (H + 15) / 16 <= FS_WO; /* (uniform) */
  float wi[FS_WI], wo[FS_WO];
  if (pre_ok) {
    const float *w = v.b.ih_w + (np < H ? np : 0);
#pragma unroll
    for (int k = 0; k < FS_WI; k++) {
      const int y = gp + Gp * k;
      wi[k] = w[(size_t)(y < I ? y : 0) * H];
    }
    const int o_ = tid & 63, g2_ = tid >> 6;
    const float *wq = v.b.ho_w + (o_ < O ? o_ : 0);
#pragma unroll
    for (int k = 0; k < FS_WO; k++) {
      const int y = g2_ + 16 * k;
      wo[k] = wq[(size_t)(y < H ? y : 0) * O];
    }
  }
  float *slot = input_row<false>(v, r, 0);
  float *hid = v.b.hidden + (size_t)r * H;
  // the input row (k_assemble, mode KEEP) and its sum
  float sum = 0.0f;
  if (tid < I) {
    float x = (tid == 0) ? 1.0f : (tid <= hs) ? hid[tid] : slot[tid];
    xs[tid] = x;
    sum = x;
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  sum = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
  {
    const float softclip = I * INPUT_MEAN_SOFT_TOP_F;
    float scale = 1.0f;
    if (sum > softclip) scale = soft_clip_dev(sum, softclip);
    if (tid < I) {
      const float x = xs[tid] * scale;
      if (sum > softclip) xs[tid] = x;
      slot[tid] = (sum > softclip) ? x : xs[tid];
    }
  }
  __syncthreads();
  // hidden sums: column n, rows y = g, g + G, ...
  const int HC = H <= 128 ? 128 : 256, G = 1024 / HC;
  const int n = tid & (HC - 1), g = tid / HC;
  float acc = 0.0f;
  if (n < H && pre_ok) {
#pragma unroll
    for (int k = 0; k < FS_WI; k++) {
      const int y = g + G * k;
      const float x = y < I ? xs[y] : 0.0f;
      acc = (x != 0.0f) ? acc + x * wi[k] : acc; /* the rows in the same order; a zero row is not multiplied */
    }
  } else if (n < H) {
    const float *w = v.b.ih_w + n;
    for (int y = g; y < I; y += G) {
      const float x = xs[y]; /* the same for the whole group: whole waves skip a zero row */
      if (x != 0.0f) acc += x * w[(size_t)y * H];
    }
  }
  part[tid] = acc;
  __syncthreads();
  if (tid < H) {
    float x = part[tid];
    for (int k = 1; k < G; k++) x += part[k * HC + tid];
    x = act_forward(s, x);
    if (tid == 0) x = 1.0f; /* the bias node, recur-nn.c:148 */
    hid[tid] = x;
    hsh[tid] = x;
  }
  __syncthreads();
  // output layer: column o, rows y = g2, g2 + 16, ...
  {
    const int o = tid & 63, g2 = tid >> 6;
    float a = 0.0f;
    if (o < O && pre_ok) {
#pragma unroll
      for (int k = 0; k < FS_WO; k++) {
        const int y = g2 + 16 * k;
        if (y < H) a += hsh[y] * wo[k];
      }
    } else if (o < O) {
      for (int y = g2; y < H; y += 16) a += hsh[y] * v.b.ho_w[(size_t)y * O + o];
    }
    part[tid] = a;
    __syncthreads();
    if (tid < O) {
      float x = part[tid];
      for (int k = 1; k < 16; k++) x += part[k * 64 + tid];
      v.b.out[(size_t)r * O + tid] = x;
    }
  }
}
