// fwd_plan.h -- which kernels a forward pass (ramd_launch_forward) gets: the rule, apart from the launches.
//
// ramd_plan_forward() reads the shape, the call's description (RamdFwdCall), a few host-side fields of RamdBuffers and
// the RECUR_AMD_* switches, and fills a FwdPlan: one form per stage -- input rows, hidden layer, presynaptic noise, the
// hidden layer's end, output layer -- with the numbers that form's launch needs.  It makes no HIP call and follows no
// device pointer (of `dense` only whether it is there), so the host compiler alone builds it and
// tests/test_fwd_plan.py asks it on a machine without a GPU.  Every switch the forward path reads is read here.
#pragma once
#include "ramd_internal.h"
#include "k_tiles.h"

enum FwdInput {
  FIN_BUILT,    /* the caller has built the rows */
  FIN_BOTTOM,   /* k_advance in front when advancing, k_bottom_forward, k_assemble keeping the layer's outputs */
  FIN_ASSEMBLE, /* k_assemble */
  FIN_INSIDE    /* the hidden layer's launch builds them (k_fwd_fused, k_fwd_small) */
};
enum FwdHidden { FH_FUSED, FH_WIDE, FH_GEMM, FH_SMALL };
enum FwdNoise {
  FN_NONE,
  FN_APPLY,   /* the values generated ahead (b->noise_spec): k_noise_apply, or inside k_fwd_finalize_fused */
  FN_GENERATE /* k_presynaptic_noise */
};
enum FwdEnd {
  FE_LEFT,           /* the sums stay in the workspace for the top launch: FwdPlan::left */
  FE_FINALIZE,       /* k_fwd_finalize over the GEMM's ks planes */
  FE_FINALIZE_FUSED, /* k_fwd_finalize_fused over k_fwd_fused's plane and its tn partials */
  FE_INSIDE          /* k_fwd_small */
};
enum FwdOutput { FO_NONE, FO_O4, FO_ROWS, FO_WIDE, FO_GEMM, FO_INSIDE };

/* a launch of k_fwd_fused<NS> (32 x 32 tiles) or k_fwd_wide<NS> (64 x 64 tiles) */
struct FwdTiles {
  int ns, tm, tn, blocks;
};

struct FwdPlan {
  FwdInput input;
  bool advance_first; /* FIN_BOTTOM: the ring's own advance launch in front */
  FwdHidden hidden;
  FwdTiles ht;        /* FH_FUSED (ns 0: any number of stages, nstages of them), FH_WIDE */
  int nstages;
  bool uniform;       /* FH_GEMM: every stream at the same ring position */
  int nkt, ks;
  FwdNoise noise;
  FwdEnd end;
  RamdHandover left;  /* FE_LEFT */
  FwdOutput output;
  FwdTiles ot;        /* FO_WIDE */
  int o_nkt, o_ks;    /* FO_GEMM */
};

/* ramd_launch_text_top takes the shape (kernels_loss.hip: ramd_text_top_ok, the question callers ask up front) */
static inline bool text_top_takes(const RamdShape *sh) {
  return sh->O <= 256 && sh->H <= 3072 && !env_int("RECUR_AMD_NO_TEXT_TOP", 0);
}

/* k_fwd_wide: 64 rows x 64 columns per workgroup with the full K (9, 17 or 33 stages of 64) in each; supertiles of
 * 4 x 8 tiles, 32 workgroups each, dealt over the 8 XCDs */
static inline bool wide_stages_ok(int K) {
  const int ns = (K + WK - 1) / WK;
  return ns == 9 || ns == 17 || ns == 33;
}
static inline FwdTiles wide_tiles(int nrows, int K, int N) {
  FwdTiles t = {(K + WK - 1) / WK, nrows / WM, (N + WN - 1) / WN, 0};
  const int supertiles = ((t.tm + 3) / 4) * ((t.tn + 7) / 8);
  t.blocks = ((supertiles + 7) / 8) * 8 * 32;
  return t;
}

/* assemble + hidden layer in one launch (k_fwd_fused): every stream at the same ring position, one-hot, text or up to
 * FF_MAXIN dense inputs, no bottom layer, hidden_size a multiple of 32, training rows */
static inline bool fwd_fused_takes(const RamdShape *sh, const RamdBuffers *b, const RamdFwdCall *c, FwdPlan *p) {
  const bool whole = c->want == RAMD_FWD_WHOLE;
  const bool dense_ok = c->mode == RAMD_IN_DENSE && c->dense && sh->input_size <= FF_MAXIN && env_int("RECUR_AMD_FWD_FUSED_DENSE", 1);
  if (b->uniform_idx < 0 || sh->bI || sh->hidden_size % CN != 0 || c->row0 + c->nrows > sh->Scap ||
      (whole ? ((c->mode != RAMD_IN_TEXT && c->mode != RAMD_IN_ONE_HOT && !dense_ok) || !env_int("RECUR_AMD_FWD_FUSED_ANY", 1))
             : ((c->mode != RAMD_IN_TEXT && !dense_ok) || !text_top_takes(sh))) ||
      env_int("RECUR_AMD_NO_FWD_FUSED", 0))
    return false;
  const int tm = (c->nrows + CM - 1) / CM, tn = sh->hidden_size / CN;
  /* dense inputs: where the 32 x 32 tiles are one round of workgroups (gstclassify's 512 / 128: 64 tiles; one launch less,
   * the time of assemble + GEMM).  Beyond that the tiles' operand traffic decides -- 8 flop per byte from L2: 67.7 us at
   * 2048 / 512 (1024 tiles) against 58.7 + 6.3 us for k_assemble and the 128 x 128 tiles of k_gemm */
  if (c->mode == RAMD_IN_DENSE && tm * tn > 256) return false;
  /* plane 0: sums; plane 1: [tn][nrows][4] padding partials */
  if ((size_t)c->nrows * sh->H + (size_t)tn * c->nrows * 4 > b->slab_floats || tn * 4 > sh->H) return false;
  p->nstages = (sh->hidden_size + CK - 1) / CK;
  const bool unrolled = sh->hidden_size % CK == 0 && (p->nstages == 2 || p->nstages == 4 || p->nstages == 8 || p->nstages == 16);
  p->ht = FwdTiles{unrolled ? p->nstages : 0, tm, tn, ((tn + 7) / 8) * 8 * tm};
  return true;
}

static inline void plan_output_layer(const RamdShape *sh, const RamdBuffers *b, int nrows, FwdPlan *p) {
  if (sh->O == 4 && nrows >= 64) {
    p->output = FO_O4;
  } else if (sh->O <= 256) {
    p->output = FO_ROWS;
  } else if (nrows % WM == 0 && sh->O >= 1024 && wide_stages_ok(sh->H) && (nrows / WM) * ((sh->O + WN - 1) / WN) >= 128 &&
             env_int("RECUR_AMD_OUT_WIDE", 1)) {
    /* wide output layers with enough tiles to fill the device (the multi-head nets: 4 x 58 at 256 streams): k_fwd_wide's
     * 64 x 64 tiles with the full K in every workgroup write `out` directly (33 + 6 us as k_gemm + k_sum_slabs) */
    p->output = FO_WIDE;
    p->ot = wide_tiles(nrows, sh->H, sh->O);
  } else { /* wide output layers (multi-head nets, O in the thousands): the MFMA GEMM */
    p->output = FO_GEMM;
    p->o_nkt = (sh->H + BK - 1) / BK;
    p->o_ks = pick_ks(((nrows + BM - 1) / BM) * ((sh->O + BN - 1) / BN), p->o_nkt, b->slab_floats, (size_t)nrows * sh->O);
  }
}

static inline FwdPlan ramd_plan_forward(const RamdShape *sh, const RamdBuffers *b, const RamdFwdCall *c) {
  FwdPlan p = {};
  const int nrows = c->nrows;
  /* (RAMD_FWD_FOR_TEXT_TOP and RAMD_FWD_FOR_DENSE_TOP plan alike: the two names say which top launch the caller makes) */
  const bool whole = c->want == RAMD_FWD_WHOLE;
  /* ---- one stream of a small net (the per-net rnn_opinion): the whole pass as one workgroup (k_fwd_small: h_size <= 256,
   * i_size <= 512, o_size <= 64; it knows neither the bottom layer nor noise) */
  if (c->one_net && nrows == 1 && whole && !sh->bI && c->noise == 0.0f && sh->H <= 256 && sh->I <= 512 && sh->O <= 64 &&
      env_int("RECUR_AMD_FWD_SMALL", 1)) {
    p.input = FIN_INSIDE, p.hidden = FH_SMALL, p.end = FE_INSIDE, p.output = FO_INSIDE;
    return p;
  }
  /* ---- input rows and hidden layer.  The fused launch: for the text step and for dense inputs on their way to
   * ramd_launch_dense_top, which take the sums as the launch leaves them (so no noise); for the one-hot and text passes
   * that go on to a generic output layer (the multi-head step) and for dense inputs (gstclassify's features, rnnca's
   * neighbourhoods; their callers advance on their own, and the index the kernel stores is the one that is there), with
   * presynaptic noise only as the values generated ahead, which the finishing kernel adds */
  if (!c->rows_built && !sh->bI && (c->advance || c->mode == RAMD_IN_DENSE) && !c->fwd_only &&
      (c->noise == 0.0f || (whole && b->noise_spec_use)) && fwd_fused_takes(sh, b, c, &p)) {
    p.input = FIN_INSIDE;
    p.hidden = FH_FUSED;
    if (whole) {
      p.noise = b->noise_spec_use ? FN_APPLY : FN_NONE;
      p.end = FE_FINALIZE_FUSED;
      plan_output_layer(sh, b, nrows, &p);
    } else {
      p.end = FE_LEFT;
      p.left = RamdHandover{1, p.ht.tn};
    }
    return p;
  }
  /* (the caller's inputs feed the bottom layer, whose rectified outputs become the real inputs of the current slot: the
   * ring has to step before it runs) */
  p.input = c->rows_built ? FIN_BUILT : sh->bI ? FIN_BOTTOM : FIN_ASSEMBLE;
  p.advance_first = p.input == FIN_BOTTOM && c->advance;
  /* (from 2048 rows: h_size = hidden_size + 4 makes 33 column tiles of 64, and with a few hundred
   * rows that 33rd tile is a second round of workgroups: 97 us against the generic kernel's 60
   * at 512 x 2048; at 13,824 rows it is 1406 us against 1515) */
  if (nrows % WM == 0 && nrows >= 2048 && wide_stages_ok(sh->I) && (size_t)nrows * sh->H <= b->slab_floats &&
      env_int("RECUR_AMD_FWD_WIDE", 1)) {
    /* big sets: 64 x 64 tiles, operands by LDS-DMA (k_fwd_wide); one plane of sums */
    p.hidden = FH_WIDE;
    p.ht = wide_tiles(nrows, sh->I, sh->H);
    p.ks = 1;
  } else {
    p.hidden = FH_GEMM;
    p.uniform = b->uniform_idx >= 0;
    p.nkt = (sh->I + BK - 1) / BK;
    p.ks = pick_ks(((nrows + BM - 1) / BM) * ((sh->H + BN - 1) / BN), p.nkt, b->slab_floats, (size_t)nrows * sh->H);
  }
  p.noise = c->noise == 0.0f ? FN_NONE : b->noise_spec_use ? FN_APPLY : FN_GENERATE;
  if (whole) {
    p.end = FE_FINALIZE;
    plan_output_layer(sh, b, nrows, &p);
  } else {
    p.end = FE_LEFT; /* the K slabs (noise included) un-summed */
    p.left = RamdHandover{p.ks, 0};
  }
  return p;
}
