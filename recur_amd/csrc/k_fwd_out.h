// k_fwd_out.h -- the output layer of rnn_opinion a row at a time: k_out_layer and k_out_layer_o4 (kernels_forward.hip
// launches them: stage_output).  Both are compiled WITHOUT fp contraction (a multiply, then an add), unlike the rest of the
// forward pass: the header sets that state for its own text and hands back the default.
#pragma once
#include "k_common.h"
#pragma clang fp contract(off)
// The output layer of rnn_opinion (recur-nn.c:150-151): out = hidden . W_ho for one state
// row per workgroup.  O is small (tens to a few hundred columns) against H, so this is
// not worth an MFMA launch plus a slab pass: thread (seg, col) walks one sixteenth of the
// hidden units down one column of W_ho (a wave reads whole contiguous rows), sixteen
// waves keep enough rows in flight to cover the L2 latency, and the segments are added
// in order.
__global__ __launch_bounds__(1024) void k_out_layer(View v, int row0) {
  extern __shared__ float osh[]; /* [H] hidden row, then [OUT_SEGS][64] partial sums */
  const RamdShape &s = v.sh;
  const int r = row0 + blockIdx.x;
  const float *hid = v.b.hidden + (size_t)r * s.H;
  for (int i = threadIdx.x; i < s.H; i += 1024) osh[i] = hid[i];
  __syncthreads();
  float *part = osh + s.H;
  const int seg = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int per = (s.H + OUT_SEGS - 1) / OUT_SEGS;
  const int y0 = seg * per, y1 = min(s.H, y0 + per);
  float *out = v.b.out + (size_t)r * s.O;
  for (int c0 = 0; c0 < s.O; c0 += 64) {
    int col = c0 + lane;
    float acc0 = 0.0f, acc1 = 0.0f;
    if (col < s.O) {
      const float *w = v.b.ho_w + col;
      int y = y0;
#pragma unroll 4
      for (; y + 1 < y1; y += 2) {
        acc0 += osh[y] * w[(size_t)y * s.O];
        acc1 += osh[y + 1] * w[(size_t)(y + 1) * s.O];
      }
      if (y < y1) acc0 += osh[y] * w[(size_t)y * s.O];
    }
    part[seg * 64 + lane] = acc0 + acc1;
    __syncthreads();
    if (seg == 0 && col < s.O) {
      float sum = part[lane];
      for (int g = 1; g < OUT_SEGS; g++) sum += part[g * 64 + lane];
      out[col] = sum;
    }
    __syncthreads();
  }
}

// The same for o_size == 4 (rnnca: Y, Cb, Cr + padding): a row of W_ho is ONE float4, so a wave
// per state row walks the hidden units 64 at a time (coalesced hidden values, coalesced float4
// weights) and reduces with xor shuffles.  k_out_layer gives every column a lane and every
// sixteenth of the rows a wave, which with 4 columns leaves 60 of 64 lanes idle: 252 us for
// the 13,824 rows of an rnnca frame at hidden 2048.
__global__ __launch_bounds__(256) void k_out_layer_o4(View v, int row0, int nrows) {
  const RamdShape &s = v.sh;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= nrows) return;
  const int r = row0 + j;
  const float *hid = v.b.hidden + (size_t)r * s.H;
  float4 acc = zero4();
  for (int y = lane; y < s.H; y += 64) {
    const float h = hid[y];
    const float4 w = ld4(v.b.ho_w + (size_t)y * 4);
    acc.x += h * w.x; acc.y += h * w.y; acc.z += h * w.z; acc.w += h * w.w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc.x += __shfl_xor(acc.x, off, 64);
    acc.y += __shfl_xor(acc.y, off, 64);
    acc.z += __shfl_xor(acc.z, off, 64);
    acc.w += __shfl_xor(acc.w, off, 64);
  }
  if (lane == 0) *reinterpret_cast<float4 *>(v.b.out + (size_t)r * 4) = acc;
}
#pragma clang fp contract(fast)
