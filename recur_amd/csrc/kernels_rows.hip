// kernels_rows.hip -- what the batched forward-only calls share on the device, as rows_host.c holds what they share on the
// host: the one launch between two forward passes of rnn_amd_run_texts and _trace_texts (texts_api.c: k_texts_step),
// rnn_amd_sample_texts and _continue_texts (sample_api.c: k_texts_continue), rnn_amd_run_sequences (seqs_api.c:
// k_seqs_step), rnn_amd_classify_texts (classify_texts_api.c: k_classify_step), rnn_amd_run_automaton (automaton_api.c:
// k_automaton_step) and rnn_amd_dream_sequences (dream_api.c: k_dream_step), and their launchers.  Every text, sequence
// or cell has a forward-only state row of the engine's own,
// one workgroup per row, and the kernels have one shape: a score,
// paint or draw half on what the forward pass just left in the row's out row, then a feed half that builds the row's next
// input row through assemble_input_row (k_common.h), on the hidden values texts_feed_hidden names.  What a launch is
// handed -- its fields and its contract -- stands once, above its struct in ramd_internal.h (the automaton's in
// automaton_rule.h, next to the rule it embeds); the kernel takes that struct by value (k_texts_step: its form's fields
// of it).
#include "k_common.h"
#include "k_top.h"
#include "sample_rule.h"
#include "continue_rule.h"
#include "automaton_rule.h"
#include "classify_rule.h"
#include "dream_rule.h"
#pragma clang fp contract(off)

constexpr int TS_WAVES = 4;
// Where the feed half of every kernel here takes state row r's hidden values from, stated once: from hid0 in a
// wave's first feed (`first`) when the call has one -- the hidden row of the net, which every row then starts from --,
// else from the row's own hidden row: what the forward pass before left there, or, with a null hid0 in the first feed,
// the start state the host has put there (the _from calls, texts_api.c and sample_api.c).
__device__ __forceinline__ const float *texts_feed_hidden(const View &v, int r, const float *hid0, bool first) {
  return first && hid0 ? hid0 : v.b.hidden + (size_t)r * v.sh.H;
}
// The score half of k_texts_step, stated once: one wave scores one head of alen outputs at src.  The wave builds the shift
// and the exponentials into ex (LDS, alen floats); behind the fence lane 0 takes their sum in the reference's order, the
// likelihood of `target` (a symbol outside the head has no probability: the cap) and returns capped log2 of it; the other
// lanes return 0.  GUESS: every lane takes the sum -- the same LDS reads, broadcast -- for softmax_best_guess's pick
// (badmaths.h:113-141: the largest likelihood after the division, the lowest index among equals): every lane offers
// ex[i] / sum for its outputs in ascending order, lanes beyond alen offer nothing, and the wave's pick is left in `guess`.
// The caller fences before the wave's next head rewrites ex.
template <bool GUESS>
__device__ __forceinline__ float texts_score_head(const float *src, float *ex, int alen, int lane, int target, int &guess) {
  wave_softmax_exps(src, ex, alen, lane, FenceOneWave{});
  if constexpr (GUESS) {
    const float sum = ordered_sum(ex, alen);
    const float l = lane == 0 ? capped_log2f_dev(target < alen ? ex[target] / sum : 0.0f) : 0.0f;
    BestGuess best;
    for (int i = lane; i < alen; i += 64) best.offer(ex[i] / sum, i);
    wave_best_guess(best);
    guess = best.i;
    return l;
  }
  if (lane == 0) {
    const float e = target < alen ? ex[target] / ordered_sum(ex, alen) : 0.0f;
    return capped_log2f_dev(e);
  }
  return 0.0f;
}
// RamdTextsStep's launch (ramd_internal.h), one workgroup per row, the heads of a row shared out over the waves.  TRACE is
// the form of rnn_amd_trace_texts; the two differ in three places: the row filter (the sums form leaves out a row before
// its skip, the trace scores every row at every step), the sink (lane 0 of the head's wave adds the float into the row's
// own double, or stores it at its place in the trace -- one writer either way: no atomics, and no memset of the trace),
// and the guess.
// The kernel's arguments are RamdTextsStep's fields of its own form, which the launcher copies out: a kernel fetches the
// arguments that lie next to text / off with them in one wide scalar load at its top, and those of the other form in
// between would push a form's own behind a second, dependent load inside its score half (profiles/r09_rows_split_rate.txt).
template <bool TRACE> struct TextsStepArgs;
template <> struct TextsStepArgs<false> {
  const unsigned char *text;
  const unsigned long long *off;
  const int *skip;
  double *acc;
  const float *hid0;
  int row0, alen, n_sums, t_score, a_score, t_feed, a_feed;
};
template <> struct TextsStepArgs<true> {
  const unsigned char *text;
  const unsigned long long *off, *off_tr;
  float *trace;
  unsigned char *guess;
  const float *hid0;
  int row0, alen, n_sums, t_score, a_score, t_feed, a_feed;
};
template <bool TRACE>
__global__ __launch_bounds__(64 * TS_WAVES) void k_texts_step(View v, TextsStepArgs<TRACE> p) {
  extern __shared__ float tex[]; /* [TS_WAVES][alen rounded up to 4] exponentials */
  __shared__ float red[4];
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = p.row0 + j, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned char *text = p.text + p.off[j];
  bool scored = j < p.a_score;
  if constexpr (!TRACE) scored = scored && p.t_score >= p.skip[j];
  if (scored) {
    const int target = text[p.t_score + 1];
    float *ex = tex + wave * ((p.alen + 3) & ~3);
    size_t at = (size_t)j * p.n_sums; /* the row's first sum, or its first traced value of this step */
    if constexpr (TRACE) at = p.off_tr[j] + (size_t)p.t_score * p.n_sums;
    for (int c = wave; c < p.n_sums; c += TS_WAVES) {
      const float *src = v.b.out + (size_t)r * s.O + (size_t)c * p.alen;
      int guess = 0;
      if constexpr (TRACE) {
        const float l = p.guess ? texts_score_head<true>(src, ex, p.alen, lane, target, guess)
                                : texts_score_head<false>(src, ex, p.alen, lane, target, guess);
        if (lane == 0) {
          p.trace[at + c] = l;
          if (p.guess) p.guess[at + c] = (unsigned char)guess;
        }
      } else {
        const float l = texts_score_head<false>(src, ex, p.alen, lane, target, guess);
        if (lane == 0) p.acc[at + c] += (double)l;
      }
      FenceOneWave{}(); /* before this wave's next head rewrites ex (the guess's reads of it have returned) */
    }
  }
  if (j < p.a_feed) /* (the whole workgroup: assemble_input_row has barriers) */
    assemble_input_row(s, input_row(v, r, 0), texts_feed_hidden(v, r, p.hid0, true), RAMD_IN_ONE_HOT, text[p.t_feed],
                       nullptr, red);
}

// RamdSeqsStep's launch (ramd_internal.h), one workgroup of 256 threads per row.  The score half is emit_opinions' loop
// body (gstclassify.c:2273-2280) on the output row the forward pass just left: a wave per class group, the groups shared
// out over the waves, lane-strided so that a group may be wider than the wave: softmax of out[goff[g] .. + gsize[g])
// (badmaths.h:71-111: the shift, fast_expf, the sum in the reference's order), every lane stores ex[i] / sum for its
// classes -- what softmax_best_guess stores, negated back -- and offers it to the best guess (badmaths.h:113-141: the
// largest after the division, the lowest index among equals), which lane 0 stores as a byte when winners are wanted.  The
// columns in no group are copied raw by the whole workgroup.  Every entry has one writer and is written once: no atomics
// and no memset.  The feed half is assemble_input_row with the staged frame as the dense row, the emergency soft clip
// included.
__global__ __launch_bounds__(64 * TS_WAVES) void k_seqs_step(View v, RamdSeqsStep p) {
  extern __shared__ float tex[]; /* [TS_WAVES][stride] exponentials */
  __shared__ float red[4];
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = p.row0 + j, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t at = (size_t)p.off[j];
  if (j < p.a_score) {
    const float *out = v.b.out + (size_t)r * s.O;
    const size_t slot = at + (size_t)p.t_score;
    float *dst = p.ans + slot * (size_t)s.output_size;
    for (int c = threadIdx.x; c < p.n_gap; c += 64 * TS_WAVES) dst[p.gap[c]] = out[p.gap[c]];
    float *ex = tex + wave * p.stride;
    for (int g = wave; g < p.n_groups; g += TS_WAVES) {
      const int o = p.goff[g], n = p.gsize[g];
      wave_softmax_exps(out + o, ex, n, lane, FenceOneWave{});
      const float sum = ordered_sum(ex, n);
      BestGuess best;
      for (int i = lane; i < n; i += 64) { /* (consecutive lanes, consecutive floats) */
        const float e = ex[i] / sum;
        dst[o + i] = e;
        best.offer(e, i);
      }
      if (p.win) {
        wave_best_guess(best);
        if (lane == 0) p.win[slot * (size_t)p.n_groups + g] = (unsigned char)best.i;
      }
      FenceOneWave{}(); /* before this wave's next group rewrites ex */
    }
  }
  if (j < p.a_feed) /* (the whole workgroup: assemble_input_row has barriers) */
    assemble_input_row(s, input_row(v, r, 0), texts_feed_hidden(v, r, p.hid0, true), RAMD_IN_DENSE, 0,
                       p.in + (at + (size_t)p.t_feed) * (size_t)s.input_size, red);
}

// RamdClassifyStep's launch (ramd_internal.h), one workgroup of 256 threads per row.  The score half is the loop body of
// text-classify-results.c:96-104 and of rnn_char_classify_epoch's validation (charmodel-classify.c:181-191) on the output
// row the forward pass just left; which rows it is for is classify_rule.h's answer.  Wave 0 builds the softmax of ALL the
// outputs as one group -- the shift and the exponentials into tex (LDS, lane-strided: output_size may exceed a wave), their
// sum in the reference's order -- and, for a symbol with a class, the best guess (badmaths.h:113-141) and the row's score,
// which lane 0 adds.  Behind the barrier the whole workgroup divides and adds: thread c's classes c, c + 256, ... into the
// row's own doubles, the square formed in float as the reference forms it.  Every word has one writer: no atomics.
__global__ __launch_bounds__(64 * TS_WAVES) void k_classify_step(View v, RamdClassifyStep p) {
  extern __shared__ float tex[]; /* [output_size] exponentials */
  __shared__ float red[4];
  __shared__ float sum_sh;
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = p.row0 + j, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t at = (size_t)p.off[j];
  /* (j < a_score: the plan's order has answered classify_fed; the same in every thread: the barrier is met by all) */
  if (j < p.a_score && classify_skip_passed(p.skip[j], p.t_score)) {
    const int n = s.output_size;
    const float *out = v.b.out + (size_t)r * s.O;
    double *acc = p.acc + (size_t)j * RAMD_CLASSIFY_ACC_WORDS(n);
    if (wave == 0) {
      wave_softmax_exps(out, tex, n, lane, FenceOneWave{});
      const float sum = ordered_sum(tex, n);
      const int cl = p.cls ? p.cls[at + (size_t)p.t_score] : CLASSIFY_NO_CLASS;
      if (classify_has_class(cl)) { /* (the same byte in every lane) */
        BestGuess best;
        for (int i = lane; i < n; i += 64) best.offer(tex[i] / sum, i);
        wave_best_guess(best);
        if (lane == 0) {
          const float e = tex[cl] / sum;
          long long *counts = reinterpret_cast<long long *>(acc + 2 * (size_t)n + 2);
          acc[2 * (size_t)n] += 1.0 - (double)e;
          acc[2 * (size_t)n + 1] -= (double)capped_log2f_dev(e);
          counts[0] += best.i == cl;
          counts[1] += 1;
        }
      }
      if (lane == 0) sum_sh = sum;
    }
    __syncthreads();
    const float sum = sum_sh;
    for (int c = threadIdx.x; c < n; c += 64 * TS_WAVES) {
      const float e = tex[c] / sum;
      const float sq = e * e;
      acc[c] += (double)e;
      acc[(size_t)n + c] += (double)sq;
    }
  }
  if (j < p.a_feed) /* (the whole workgroup: assemble_input_row has barriers) */
    assemble_input_row(s, input_row(v, r, 0), texts_feed_hidden(v, r, p.hid0, true), RAMD_IN_ONE_HOT,
                       p.text[at + (size_t)p.t_feed], nullptr, red);
}

// RamdAutomatonStep's launch (automaton_rule.h): rnnca's fill_frame (gstrnnca.c:805-831) with a forward-only state row per
// cell, all width * height of them in lock step.  One workgroup of 256 threads per cell (assemble_input_row's).  The paint
// half is three threads, a byte each: one writer per byte, no atomics and no memset.  The feed half puts the cell's dense
// input row into LDS -- the levels of its neighbours in the frame before, the position -- and calls assemble_input_row
// with it, the emergency soft clip included.
// A cell's feed needs its neighbours' levels of the very frame this launch paints, and those bytes are other workgroups'
// writes of this launch: reading them back would be a race.  So the feed half does not read the frame: it reads the
// neighbours' OUT rows, which no workgroup of this launch writes, and applies the same level function -- at most
// len_y + 2 * len_c small evaluations per cell, and the same byte as the one painted because the rule is stated once.
// Only a call's first launch (seed != nullptr) gathers bytes: the seed frame's, which no launch writes.
struct AutomatonExp {
  __device__ __forceinline__ float operator()(float x) const { return fast_expf_dev(x); }
};
struct AutomatonSeedLevels { /* the frame before is bytes in memory */
  const unsigned char *frame;
  int cells;
  __device__ __forceinline__ unsigned char operator()(int plane, int cell) const {
    return frame[(size_t)plane * cells + cell];
  }
};
struct AutomatonOutLevels { /* the frame before is what the cells' out rows paint */
  const float *out; /* cell 0's out row */
  int O;
  __device__ __forceinline__ unsigned char operator()(int plane, int cell) const {
    return automaton_level(out[(size_t)cell * O + plane], AutomatonExp{});
  }
};
__global__ __launch_bounds__(256) void k_automaton_step(View v, RamdAutomatonStep p) {
  extern __shared__ float cell_in[]; /* [input_size] the cell's dense input row */
  __shared__ float red[4];
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = p.row0 + j;
  const int cells = p.g.width * p.g.height;
  const float *out0 = v.b.out + (size_t)p.row0 * s.O;
  if (p.paint && threadIdx.x < 3)
    p.paint[(size_t)threadIdx.x * cells + j] = automaton_level(out0[(size_t)j * s.O + threadIdx.x], AutomatonExp{});
  if (p.feed) { /* (the whole workgroup: barriers) */
    const int cx = j % p.g.width, cy = j / p.g.width;
    if (p.seed) {
      const AutomatonSeedLevels level = {p.seed, cells};
      for (int i = threadIdx.x; i < s.input_size; i += 256) cell_in[i] = automaton_input(p.g, cx, cy, i, level);
    } else {
      const AutomatonOutLevels level = {out0, s.O};
      for (int i = threadIdx.x; i < s.input_size; i += 256) cell_in[i] = automaton_input(p.g, cx, cy, i, level);
    }
    __syncthreads();
    assemble_input_row(s, input_row(v, r, 0), texts_feed_hidden(v, r, p.hid0, true), RAMD_IN_DENSE, 0, cell_in, red);
  }
}

// RamdDreamStep's launch (ramd_internal.h): parrot's player (fill_audio_chunk, gstparrot.c:556-583) with a forward-only
// state row per sequence, all of them in lock step.  One workgroup of 256 threads per row (assemble_input_row's).  Thread
// i, i + 256, .. applies dream_tanh to the row's own out[i], stores it at its place in the segment's buffer and forms
// dream_next of it with the frame's draw gz[i][row] into LDS: the dense row that assemble_input_row takes, the emergency
// soft clip included -- or, in a call's last launch, into the row of `next`.  The tanh that is fed is the one that was
// emitted, from the thread's register: nothing another workgroup writes is read.
__global__ __launch_bounds__(256) void k_dream_step(View v, RamdDreamStep p) {
  extern __shared__ float dream_in[]; /* [input_size] the row's dense input row */
  __shared__ float red[4];
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = p.row0 + j, n = s.output_size;
  if (p.first) { /* (the same in every thread: the whole workgroup, assemble_input_row has barriers) */
    assemble_input_row(s, input_row(v, r, 0), texts_feed_hidden(v, r, p.hid0, true), RAMD_IN_DENSE, 0,
                       p.first + (size_t)j * p.ld_first, red);
    return;
  }
  const bool draws = dream_draws(p.noise);
  const float *out = v.b.out + (size_t)r * s.O;
  const float *gz = p.gz + j; /* the row's column of gz[output_size][rows] (not read without draws) */
  float *emit = p.emit + (size_t)j * n;
  float *dst = p.next ? p.next + (size_t)j * n : dream_in;
  for (int i = threadIdx.x; i < n; i += 256) { /* (element i is read and written by this thread alone) */
    const float a = dream_tanh(out[i]);
    emit[i] = a;
    dst[i] = draws ? dream_next(a, p.noise, gz[(size_t)i * p.rows]) : a;
  }
  if (p.next) return;
  __syncthreads();
  assemble_input_row(s, input_row(v, r, 0), texts_feed_hidden(v, r, nullptr, false), RAMD_IN_DENSE, 0, dream_in, red);
}
// One frame's draws of rnn_amd_dream_sequences, ahead of the launch that takes them (ramd_launch_dream_draw): a
// generator is a recurrence -- 3 rand64 per value, one lane per row whatever the number of rows -- so it runs on the side
// stream beside the forward passes, as the presynaptic noise does (noise_ahead.c).  Lane k of the grid is row k: n values
// in index order into gz[0 .. n)[k] -- value-major, so that a wave's 64 lanes store 64 consecutive floats (row-major, 64
// separate lines a store, measured the same: 58.1 against 57.2 us a frame, profiles/r13_dream_rate.txt) --, the generator
// stored back.
struct DreamGaussian {
  Rng32 &r;
  __device__ __forceinline__ float operator()() { return dev_cheap_gaussian_pair(r); }
};
__global__ __launch_bounds__(64) void k_dream_draw(DevRng *rng, float *gz, int rows, int n) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= rows) return;
  Rng32 r32 = rng_split(rng[k]);
  DreamGaussian gaussian = {r32};
  dream_draw(gz + k, n, (size_t)rows, gaussian);
  rng_join(rng[k], r32);
}

struct SampleWave { /* sample_rule.h's team: the 64 lanes of one wave */
  int l;
  __device__ __forceinline__ int lane() const { return l; }
  __device__ __forceinline__ int stride() const { return 64; }
  __device__ __forceinline__ void extremes(float &lo, float &hi) const { wave_minmax(lo, hi); }
  __device__ __forceinline__ void fence() const { FenceOneWave{}(); }
};
struct SampleExp {
  __device__ __forceinline__ float operator()(float x) const { return fast_expf_dev(x); }
};
struct SampleRand64 {
  DevRng &g;
  __device__ __forceinline__ unsigned long long operator()() { return dev_rand64(g); }
};
// The draw half of k_texts_continue: the whole of wave 0 calls it for a row that is not done.  The wave turns the row's
// slice of the output row into the distribution in sdist (LDS, alen floats); lane 0 draws from it with rng[j], stores the
// pick as symbol `idx` of the row's text, the count idx + 1 and the generator, and sets done[j] (1: the pick was
// stop_point, 2: the draw met the attempt cap and nothing was stored).  Returns, in lane 0, the pick if the row runs on,
// else -1; in the other lanes -1.
__device__ __forceinline__ int texts_draw_and_store(const View &v, int r, int j, int lane, float *sdist, DevRng *rng,
                                                    unsigned char *text, int *len, int *done, int alen, int head,
                                                    int max_len, int idx, int stop_point, float bias) {
  const float *score = v.b.out + (size_t)r * v.sh.O + (size_t)head * alen;
  const bool greedy = bias >= SAMPLE_GREEDY_BIAS;
  if (!greedy) sample_distribution(sdist, score, alen, bias, SampleExp{}, SampleWave{lane});
  int hot = -1;
  if (lane == 0) {
    int pick;
    if (greedy) {
      pick = sample_greedy(score, alen);
    } else {
      DevRng g = rng[j];
      SampleRand64 draw = {g};
      pick = sample_draw(sdist, alen, draw);
      rng[j] = g;
    }
    if (pick == SAMPLE_FAILED) {
      done[j] = 2;
    } else {
      text[(size_t)j * max_len + idx] = (unsigned char)pick;
      len[j] = idx + 1;
      if (pick == stop_point) done[j] = 1;
      else hot = pick;
    }
  }
  return hot;
}

// RamdTextsContinue's launch (ramd_internal.h), one workgroup of 256 threads per row (assemble_input_row's).  What launch t
// is for a row -- feeding a prompt symbol, drawing a text index, or nothing -- is continue_rule.h's answer for the row's
// plen (with `first`: 1).  Wave 0 fetches the prompt symbol or draws (texts_draw_and_store); the symbol reaches the
// workgroup through LDS behind a barrier.  A row that is done or idle is not fed: its input row stays what it was and the
// forward passes that follow recompute what they computed.  Every word has one writer: no atomics.
__global__ __launch_bounds__(256) void k_texts_continue(View v, RamdTextsContinue p) {
  extern __shared__ float sdist[]; /* [alen] the row's distribution */
  __shared__ float red[4];
  __shared__ int hot_sh; /* the symbol to feed, or -1 */
  const RamdShape &s = v.sh;
  const int j = blockIdx.x, r = p.row0 + j, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const ContinueStep st = continue_step(p.first ? 1 : p.plen[j], p.max_len, p.t); /* (the same in every thread) */
  if (wave == 0) {
    int hot = -1;
    if (st.what == CONTINUE_PROMPT) {
      hot = p.first ? p.first[j] : p.prompt[p.off[j] + st.index];
    } else if (st.what == CONTINUE_DRAW && p.done[j] == 0) { /* (the same word in every lane: the wave takes one side) */
      hot = texts_draw_and_store(v, r, j, lane, sdist, (DevRng *)p.rng, p.text, p.len, p.done, p.alen, p.head, p.max_len,
                                 st.index, p.stop_point, p.bias);
    }
    if (lane == 0) hot_sh = st.feeds ? hot : -1;
  }
  __syncthreads();
  const int hot = hot_sh;
  if (hot >= 0) /* (the whole workgroup: assemble_input_row has barriers) */
    assemble_input_row(s, input_row(v, r, 0), texts_feed_hidden(v, r, p.hid0, st.on_hid0), RAMD_IN_ONE_HOT, hot, nullptr,
                       red);
}

#pragma clang fp contract(fast)

// What the launchers share.  The kernels write forward-only input rows (the automaton's also reads every cell's out row):
// rows row0 .. row0 + rows are such rows, or abort naming `who`
static void forward_rows_or_abort(const char *who, const RamdShape *sh, int row0, long long rows) {
  if (rows < 1 || row0 < sh->Scap || row0 + rows > sh->Scap + sh->Fcap) {
    fprintf(stderr, "librecur_amd: %s: rows %d .. %lld are not forward-only state rows\n", who, row0, row0 + rows);
    abort();
  }
}
// `floats` floats of LDS for KERNEL's softmax over `outputs` outputs, in bytes: they fit, or abort; above 64 KiB the
// kernel's limit is raised
template <auto KERNEL>
static size_t softmax_lds_or_abort(size_t floats, int outputs) {
  const size_t shm = floats * sizeof(float);
  if (shm > 160 * 1024 - 64) {
    fprintf(stderr, "librecur_amd: a softmax over %d outputs does not fit the LDS\n", outputs);
    abort();
  }
  if (shm > 64 * 1024) raise_lds_limit<KERNEL>(160 * 1024 - 64);
  return shm;
}

template <bool TRACE>
static void launch_texts_step(hipStream_t st, const RamdShape *sh, const RamdBuffers *b, const TextsStepArgs<TRACE> &p,
                              int rows) {
  const size_t shm = softmax_lds_or_abort<k_texts_step<TRACE>>((size_t)TS_WAVES * ((p.alen + 3) & ~3), p.alen);
  RAMD_LAUNCH(k_texts_step<TRACE>, dim3(rows), dim3(64 * TS_WAVES), shm, st, make_view(sh, b), p);
}
extern "C" void ramd_launch_texts_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, const RamdTextsStep *p) {
  const int rows = p->a_score > p->a_feed ? p->a_score : p->a_feed;
  if (rows < 1) return;
  if (!p->trace) {
    forward_rows_or_abort("ramd_launch_texts_step", sh, p->row0, rows);
    launch_texts_step<false>((hipStream_t)st, sh, b, {p->text, p->off, p->skip, p->acc, p->hid0, p->row0, p->alen, p->n_sums,
                                                      p->t_score, p->a_score, p->t_feed, p->a_feed}, rows);
    return;
  }
  forward_rows_or_abort("ramd_launch_texts_step (trace)", sh, p->row0, rows);
  if (p->alen < 1 || p->n_sums < 1 || (size_t)p->n_sums * p->alen > (size_t)sh->O || (p->a_score > 0 && p->t_score < 0)) {
    fprintf(stderr, "librecur_amd: ramd_launch_texts_step (trace): %d heads of %d outputs in a row of %d, step %d\n",
            p->n_sums, p->alen, sh->O, p->t_score);
    abort();
  }
  launch_texts_step<true>((hipStream_t)st, sh, b, {p->text, p->off, p->off_tr, p->trace, p->guess, p->hid0, p->row0, p->alen,
                                                   p->n_sums, p->t_score, p->a_score, p->t_feed, p->a_feed}, rows);
}

extern "C" void ramd_launch_seqs_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, const RamdSeqsStep *p_) {
  RamdSeqsStep p = *p_;
  const int rows = p.a_score > p.a_feed ? p.a_score : p.a_feed;
  if (rows < 1) return;
  forward_rows_or_abort("ramd_launch_seqs_step", sh, p.row0, rows);
  if (p.n_groups < 0 || p.n_gap < 0 || p.largest < 0 || p.largest > sh->output_size || p.n_gap > sh->output_size ||
      (p.n_groups > 0 && (!p.goff || !p.gsize || p.largest < 1)) || (p.n_gap > 0 && !p.gap) || (p.win && p.n_groups < 1) ||
      (p.a_score > 0 && (p.t_score < 0 || !p.ans)) || (p.a_feed > 0 && (p.t_feed < 0 || !p.in)) || !p.off) {
    fprintf(stderr, "librecur_amd: ramd_launch_seqs_step: %d groups of up to %d and %d other columns in a row of %d, "
                    "steps %d and %d\n", p.n_groups, p.largest, p.n_gap, sh->output_size, p.t_score, p.t_feed);
    abort();
  }
  const int largest = p.largest;
  p.stride = (largest + 3) & ~3; /* (over `largest`, in this copy) */
  const size_t shm = softmax_lds_or_abort<k_seqs_step>((size_t)TS_WAVES * p.stride, largest);
  RAMD_LAUNCH(k_seqs_step, dim3(rows), dim3(64 * TS_WAVES), shm, (hipStream_t)st, make_view(sh, b), p);
}

extern "C" void ramd_launch_classify_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                                          const RamdClassifyStep *p) {
  const int rows = p->a_score > p->a_feed ? p->a_score : p->a_feed;
  if (rows < 1) return;
  forward_rows_or_abort("ramd_launch_classify_step", sh, p->row0, rows);
  if (sh->output_size < 1 || !p->off || (p->a_score > 0 && (p->t_score < 0 || !p->acc || !p->skip)) ||
      (p->a_feed > 0 && (p->t_feed < 0 || !p->text))) {
    fprintf(stderr, "librecur_amd: ramd_launch_classify_step: %d outputs, steps %d and %d for %d and %d rows\n",
            sh->output_size, p->t_score, p->t_feed, p->a_score, p->a_feed);
    abort();
  }
  const size_t shm = softmax_lds_or_abort<k_classify_step>((size_t)((sh->output_size + 3) & ~3), sh->output_size);
  RAMD_LAUNCH(k_classify_step, dim3(rows), dim3(64 * TS_WAVES), shm, (hipStream_t)st, make_view(sh, b), *p);
}

extern "C" void ramd_launch_automaton_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                                           const RamdAutomatonStep *p) {
  const AutomatonRule *grid = &p->g;
  const long long cells = grid->width < 1 || grid->height < 1 ? 0 : (long long)grid->width * grid->height;
  if (!p->paint && !p->feed) return;
  forward_rows_or_abort("ramd_launch_automaton_step", sh, p->row0, cells); /* (a grid without a cell has no rows) */
  if (grid->len_y < 0 || grid->len_c < 0 || (grid->len_y > 0 && !grid->offsets_y) || (grid->len_c > 0 && !grid->offsets_c) ||
      automaton_input_size(grid) != sh->input_size || sh->output_size < 3) {
    fprintf(stderr, "librecur_amd: ramd_launch_automaton_step: %d + 2 * %d + %d inputs for a net of %d, %d outputs\n",
            grid->len_y, grid->len_c, grid->len_pos, sh->input_size, sh->output_size);
    abort();
  }
  const size_t shm = (size_t)((sh->input_size + 3) & ~3) * sizeof(float);
  if (shm > 64 * 1024) {
    fprintf(stderr, "librecur_amd: a cell's %d inputs do not fit the LDS\n", sh->input_size);
    abort();
  }
  RAMD_LAUNCH(k_automaton_step, dim3((unsigned)cells), dim3(256), shm, (hipStream_t)st, make_view(sh, b), *p);
}

extern "C" void ramd_launch_dream_step(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b, const RamdDreamStep *p) {
  if (p->rows < 1) return;
  forward_rows_or_abort("ramd_launch_dream_step", sh, p->row0, p->rows);
  if (sh->input_size != sh->output_size || sh->output_size < 1 || (p->first && p->ld_first < sh->input_size) ||
      (!p->first && (!p->emit || (dream_draws(p->noise) && !p->gz)))) {
    fprintf(stderr, "librecur_amd: ramd_launch_dream_step: %d inputs and %d outputs, first rows of %d floats, or a NULL "
                    "frame or draw array\n", sh->input_size, sh->output_size, p->ld_first);
    abort();
  }
  const size_t shm = (size_t)((sh->input_size + 3) & ~3) * sizeof(float);
  if (shm > 64 * 1024) {
    fprintf(stderr, "librecur_amd: a dream's %d inputs do not fit the LDS\n", sh->input_size);
    abort();
  }
  RAMD_LAUNCH(k_dream_step, dim3(p->rows), dim3(256), shm, (hipStream_t)st, make_view(sh, b), *p);
}

extern "C" void ramd_launch_dream_draw(ramd_stream_t st, void *rng, float *gz, int rows, int n) {
  if (rows < 1 || n < 1) return;
  if (!rng || !gz) {
    fprintf(stderr, "librecur_amd: ramd_launch_dream_draw: a NULL generator or draw array for %d rows of %d\n", rows, n);
    abort();
  }
  RAMD_LAUNCH(k_dream_draw, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)st, (DevRng *)rng, gz, rows, n);
}

extern "C" void ramd_launch_texts_continue(ramd_stream_t st, const RamdShape *sh, const RamdBuffers *b,
                                           const RamdTextsContinue *p) {
  if (p->rows < 1) return;
  forward_rows_or_abort("ramd_launch_texts_continue", sh, p->row0, p->rows);
  if (p->alen < 1 || p->head < 0 || (size_t)(p->head + 1) * p->alen > (size_t)sh->O || p->t < 0 || p->max_len < 1) {
    fprintf(stderr, "librecur_amd: ramd_launch_texts_continue: head %d of %d outputs in a row of %d, step %d, texts of %d\n",
            p->head, p->alen, sh->O, p->t, p->max_len);
    abort();
  }
  const size_t shm = softmax_lds_or_abort<k_texts_continue>((size_t)((p->alen + 3) & ~3), p->alen);
  RAMD_LAUNCH(k_texts_continue, dim3(p->rows), dim3(256), shm, (hipStream_t)st, make_view(sh, b), *p);
}
