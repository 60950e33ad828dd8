// calc_plan.h -- which kernels a call of ramd_launch_calc_deltas gets: the rule, apart from the launches.
//
// ramd_plan_calc_deltas() reads the shape, the call's arguments, a few host-side fields of RamdBuffers and of the
// caller's RamdPendingDelta and the RECUR_AMD_* switches, and fills a CalcPlan.  It makes no HIP call and follows no
// device pointer (of ranges, active, ho_slab, mheads_part and own_slab only whether they are there), so the host
// compiler alone builds it and tests/test_calc_plan.py asks it on a machine without a GPU.  What depends on the
// chain launch's answer is planned after it: ramd_plan_ho_gemm() and ramd_plan_delta_dma().
#pragma once
#include "ramd_internal.h"
#include "k_tiles.h"

constexpr int DNW = 8, DP = 5; /* k_delta_direct: waves per workgroup, K quads in flight per wave */

enum CalcTop { TOP_DONE, TOP_SPARSE, TOP_HEADS, TOP_RANGED, TOP_PLAIN };
enum CalcXcRequest { XC_NONE, XC_GATHER, XC_DENSE };
enum CalcExtras { XF_CONTROL5, XF_CONTROL8, XF_CONTROL9, XF_DENSE, XF_GEMM };

struct CalcPlan {
  /* top backprop */
  bool writeback_first; /* the error images are rebuilt in front (RAMD_IMAGES_PENDING) ... */
  unsigned flags;       /* ... and the flags of everything after say so */
  CalcTop top;
  int top_nb; /* partial sums per stream in the workspace (TOP_HEADS, TOP_RANGED) */
  /* weight-delta GEMM: its form is known before the first launch, the earlier stages ask */
  bool dma, has_rest;
  bool direct, direct_runs, direct_fuse; /* (direct_runs: and the planes of a K split fit the workspace) */
  int dtm, dtn, drest, npw, drg, dn_it, dks, fast_its;
  /* top layer's delta: in k_delta_direct's first microseconds, or asked of the chain launch, else ramd_plan_ho_gemm */
  bool ho_in_delta, ho_asked;
  bool small; /* k_bptt_small takes the call */
  size_t small_lds;
  /* extras and control */
  int nx, nxp, tn;      /* column 0 + the input columns (padded); the control kernel's column tiles */
  CalcXcRequest xc_req; /* asked of the chain launch */
  CalcExtras extras;    /* where the chain declines */
  int xks;              /* XF_GEMM's K split */
  /* generic GEMMs (and what the delta stage's forms share) */
  bool own_ws; /* planes go to the caller's workspace */
  size_t slab_floats, n;
  int rtiles, nkt, ks;
  bool big;
};

/* row tiles of k_delta_direct that make whole rounds of 256 workgroups, or nearly */
static inline bool dd_rounds_ok(int tm, int tn) {
  const int tiles = tm * tn, rounds = (tiles + 255) / 256;
  return tiles >= 192 && 10 * tiles >= 9 * 256 * rounds;
}

static inline bool ranges_are_heads(const RamdBuffers *b, bool ranges, int range_stride, unsigned flags) {
  return ranges && range_stride && (flags & RAMD_RANGES_ARE_HEADS) && b->mheads_alen >= 24 && b->mheads_alen <= 128;
}

static inline CalcPlan ramd_plan_calc_deltas(const RamdShape *sh, const RamdBuffers *b, int row0, int nrows, int accumulate,
                                             bool ranges, int range_stride, bool active, unsigned flags,
                                             const RamdPendingDelta *defer, bool half_hook) {
  CalcPlan p = {};
  /* ---- top backprop */
  const int alen = b->mheads_alen, ncls = alen > 0 ? sh->output_size / alen : 0;
  const bool top_sparse = !(flags & RAMD_TOP_DONE) && ranges_are_heads(b, ranges, range_stride, flags) && ncls <= 64 &&
                          sh->output_size == ncls * alen && b->mheads_part &&
                          (size_t)sh->Scap * ncls * sh->H <= b->mheads_part_floats && row0 + nrows <= sh->Scap &&
                          env_int("RECUR_AMD_TOP_SPARSE", 1);
  /* (k_top_heads_combine takes the images' stale entries from the planes itself) */
  p.writeback_first = (flags & RAMD_IMAGES_PENDING) && !(top_sparse && env_int("RECUR_AMD_STALE_FROM_PLANES", 1));
  if (p.writeback_first) flags &= ~RAMD_IMAGES_PENDING;
  p.flags = flags;
  if (flags & RAMD_TOP_DONE) { /* ramd_launch_text_top has already done the top backprop */
    p.top = TOP_DONE;
  } else if (top_sparse) {
    p.top = TOP_SPARSE;
  } else if (ranges && range_stride && (flags & RAMD_RANGES_ARE_HEADS) && sh->O % 4 == 0 && sh->O >= 64 &&
             (size_t)nrows * 2 * ((sh->H + 31) / 32) <= b->slab_floats && env_int("RECUR_AMD_TOP_HEADS", 1)) {
    p.top = TOP_HEADS;
    p.top_nb = 2 * ((sh->H + 31) / 32);
  } else if (ranges && env_int("RECUR_AMD_TOP_RANGED", 1)) {
    /* up to 16 workgroups per stream (their partial sums sit in the split-K workspace, which
     * nothing uses at this point) */
    /* (measured: 256 streams with 1 / 2 / 4 / 8 / 16 workgroups per stream = 552 / 548 / 538 /
     * 550 / 629 us per generation; 64 streams with 4 / 16: 347 / 358; 32 streams with 8 / 16: 306 / 312) */
    int nb = 256 / nrows;
    if (nb < 4) nb = nrows > 1024 ? 1 : 4;
    if (nb > 16) nb = 16;
    if ((size_t)nrows * nb > b->slab_floats) nb = 1;
    p.top = TOP_RANGED;
    p.top_nb = nb;
  } else
    p.top = TOP_PLAIN;

  /* ---- the weight-delta GEMM's path: when it ends with the small GEMM over the rows above the last whole 128-row
   * tile, the top layer's equally small delta GEMM can share that launch (nothing before the optimiser needs its result) */
  p.dma = b->uniform_idx >= 0 && nrows % BK == 0 && sh->hidden_size % 128 == 0 && sh->I >= 128 && sh->activation != 5 &&
          env_int("RECUR_AMD_DELTA_DMA", 1);
  p.has_rest = p.dma && (sh->I / 128) * 128 < sh->I;
  /* k_delta_direct.  Row tiles: as many whole ones as make whole rounds of 256 workgroups, or nearly -- a multi-head
   * net's 1100 input rows are 17 x 16 = 272 tiles, a round of 256 and a round of 16: twice the time; as 16 row tiles
   * they are one round with 76 rest rows, two pieces of them per workgroup (NPW) */
  p.dtn = sh->hidden_size / 64;
  p.dtm = sh->I / 64;
  if (!dd_rounds_ok(p.dtm, p.dtn) && p.dtm > 16 && sh->I - 64 * (p.dtm - 1) <= 128 && dd_rounds_ok(p.dtm - 1, p.dtn)) p.dtm--;
  p.drest = sh->I - 64 * p.dtm;
  /* the rest rows' pieces: 16 per column tile (up to 64 rest rows) or 32, one or two per workgroup of the tile's first
   * 16 row tiles -- or two per workgroup where there are only 8 row tiles (hidden 512) */
  p.npw = p.dtm >= 16 ? (p.drest > 64 ? 2 : 1) : 2;
  p.drg = p.dtm >= 16 ? 4 * p.npw : 4;
  const int qps = nrows / 4;
  p.dn_it = qps % DNW == 0 ? sh->D * (qps / DNW) : -1;
  /* fewer tiles than that (hidden 512: 8 x 8): K split two or four ways over workgroups, the parts' sums as planes for the
   * optimiser's launch (or k_delta_finalize) to add -- what k_delta_dma leaves, from 64 x 64 tiles without LDS staging:
   * 43.5 -> ... us at 512 / 128 / 30 */
  const bool rounds_ok = dd_rounds_ok(p.dtm, p.dtn);
  const int dtiles = p.dtm * p.dtn;
  p.dks = 1;
  if (!rounds_ok && p.dn_it > 0 && env_int("RECUR_AMD_DELTA_DIRECT_SPLIT", 1))
    for (int k = 4; k >= 2 && p.dks == 1; k -= 2)
      if (dtiles * k >= 192 && dtiles * k <= 256 && p.dn_it % (k * DP) == 0 && p.dn_it / k >= DP) p.dks = k;
  p.direct = b->uniform_idx >= 0 && sh->hidden_size % 64 == 0 && p.dtn > 0 && (rounds_ok || p.dks > 1) &&
             (p.drest == 0 || (p.dtm >= 16 && p.drest <= 128) || (p.dtm >= 8 && p.drest <= 64)) && nrows % (4 * DNW) == 0 &&
             nrows <= 256 * (DD_FLAG_LOADS / 2) && row0 + nrows <= sh->Scap && sh->activation != 5 && p.dn_it >= DP &&
             p.dn_it % DP == 0 && !(half_hook && env_int("RECUR_AMD_DIST_OVERLAP", 0)) && env_int("RECUR_AMD_DELTA_DIRECT", 1);
  p.direct_fuse = p.direct && p.dks == 1 && defer && defer->fuse_want && !accumulate &&
                  !(flags & (RAMD_NO_HO_DELTA | RAMD_IH_SCALE_IN_RATE));
  /* ---- the top layer's delta.  When k_delta_direct carries the update, delta and update ride in ITS first
   * microseconds (HoWork's preconditions: up to 256 streams, o_size <= 48, five rows of ho_delta per workgroup at most) */
  /* (not where the chain launch has workgroups without chain work -- half of it or more, chain_plan.h: chain_segment's
   * idle_only: there the request costs the chain nothing, here it costs 2.4 us: the 48 loads per wave queue behind the
   * ring's at the CU's 64 bytes per clock.  256 streams at hidden 1024: chain 107.6 -> 104.1 us, this launch 91.9 -> 94.3,
   * generation 221.0 -> 219.9.  They are two rules, not one: this one counts 32-stream row tiles whatever tiles the chain
   * picks, so at hidden 1024 with 128 streams the two differ) */
  p.ho_in_delta = p.direct_fuse && defer->fuse_method == 0 && !ranges && !active && nrows >= 16 && nrows <= 256 &&
                  sh->O <= 48 && sh->O % 4 == 0 && sh->H <= 5 * dtiles && (nrows / 32) * (sh->hidden_size / 32) > 128 &&
                  env_int("RECUR_AMD_HO_IN_DELTA", 1);
  /* Otherwise, where the one-launch chain will run, it is handed to that launch as a request (HoWork: formed while the
   * chain's weight panels are on their way, no launch of its own) */
  /* (up to 256 streams: the request costs the chain launch 0.014 us per stream -- 3.6 us at 256 against the GEMM's
   * 6.2 us launch -- and nothing where the set leaves workgroups of that launch without chain work: 32 streams
   * 145.3 -> 141.0 us per generation, 64: 155.7 -> 151.2, 256: 244.8 -> 242.4) */
  p.ho_asked = !p.ho_in_delta && !(flags & RAMD_NO_HO_DELTA) && !ranges && !accumulate && nrows >= 16 && nrows <= 256 &&
               sh->O <= 48 && env_int("RECUR_AMD_HO_IN_CHAIN", 1);

  /* ---- one stream of a small net (the per-net calls): chain, extras, control and weight deltas in one workgroup.
   * h_size <= 128 and i_size <= 256 (text-predict's default 99 hidden units: 100 x 142): the matrix lives in the
   * workgroup's registers; larger nets take the launch-per-step route */
  p.nx = sh->I - sh->hidden_size;
  p.nxp = ramd_nxp(sh);
  p.tn = (sh->hidden_size + CN - 1) / CN;
  p.small_lds = (size_t)(128 + 256 + 256 + 20 + ((sh->D + 3) & ~3) + (size_t)sh->D * sh->I) * sizeof(float);
  p.small = nrows == 1 && !active && row0 < sh->Scap && sh->H <= 256 && env_int("RECUR_AMD_BPTT_SMALL", 1) && sh->H <= 128 &&
            sh->I <= 256 && p.small_lds <= 150 * 1024;
  if (p.small) return p;

  /* ---- extras and control ride in the one-launch chain's tail where they are the gather form (XcWork, k_common.h) or,
   * for dense inputs (gstclassify's features), a small GEMM there (extras_dense_tail) */
  const bool gather = sh->H <= 2304 && !(b->dense_inputs && p.nx > 8);
  const bool planes_31 = (size_t)(sh->D + 1) * sh->Scap * sh->I * sizeof(float) < ((size_t)1 << 31); /* (32-bit byte offsets into the planes) */
  if (gather && p.nx <= 128 && env_int("RECUR_AMD_XC_IN_CHAIN", 1) && planes_31)
    p.xc_req = XC_GATHER;
  else if (b->dense_inputs && p.nx > 8 && p.nx <= 16 * XD_NT && (sh->hidden_size == 512 || sh->hidden_size == 1024) &&
           sh->D <= 63 && env_int("RECUR_AMD_XC_IN_CHAIN", 1) && env_int("RECUR_AMD_XC_DENSE_IN_CHAIN", 1) && planes_31)
    p.xc_req = XC_DENSE;
  /* where the chain declines: the gather over the non-zero input rows (one-hot symbols: two rows per step and stream),
   * extras and control in one launch; for dense inputs with more than a handful of columns the GEMM over all of them */
  const int M = sh->D * nrows, nq = (sh->H / 4 + 63) / 64;
  p.xks = pick_ks(((M + BM - 1) / BM) * ((p.nx + BN - 1) / BN), (sh->H + BK - 1) / BK, b->slab_floats, (size_t)M * p.nxp);
  if (gather)
    p.extras = nq <= 5 ? XF_CONTROL5 : nq <= 8 ? XF_CONTROL8 : XF_CONTROL9; /* (9: h_size 2052, hidden 2048) */
  else if (p.nx <= 16 * XD_NT && env_int("RECUR_AMD_EXTRAS_DENSE", 1))
    p.extras = XF_DENSE; /* up to 47 dense inputs: GEMM and finalize in one launch */
  else
    p.extras = XF_GEMM; /* very wide nets */

  /* ---- weight deltas: one GEMM over (step, stream).  Planes that are to outlive the call go to the caller's workspace */
  p.own_ws = defer && defer->own_slab && !accumulate;
  p.slab_floats = p.own_ws ? defer->own_slab_floats : b->slab_floats;
  /* only columns 1..hidden_size of the delta can be non-zero (h_error[0] and the pad are zero, recur-nn.c:334-337), so
   * the column tiles start at 1: at hidden 1024 that is 16 exact tiles instead of 17 */
  p.rtiles = (nrows + BK - 1) / BK;
  p.nkt = sh->D * p.rtiles;
  p.n = (size_t)sh->I * sh->H;
  p.big = sh->I >= 256 && p.nkt >= 16;
  p.ks = p.big ? pick_ks(((sh->I + BM2 - 1) / BM2) * ((sh->hidden_size + BN2 - 1) / BN2), p.nkt, p.slab_floats, p.n)
               : pick_ks(((sh->I + BM - 1) / BM) * ((sh->hidden_size + BN - 1) / BN), p.nkt, p.slab_floats, p.n);
  p.direct_runs = p.direct && (p.dks == 1 || (size_t)p.dks * p.n <= p.slab_floats);
  if (p.direct_runs) { /* the shares of a SIMD's two waves (dd_body): 5 / 8 to the first where the loop is long, rounded to whole rings */
    const int pct = env_int("RECUR_AMD_DELTA_FAST_PCT", 66), n_pair = 2 * (p.dn_it / p.dks);
    if (pct > 0 && p.dn_it / p.dks >= 40) {
      int nf = (n_pair * pct / 100 + DP / 2) / DP * DP;
      if (nf < DP) nf = DP;
      if (nf > n_pair - DP) nf = n_pair - DP;
      p.fast_its = nf;
    }
  }
  return p;
}

/* The top layer's delta where neither k_delta_direct nor the chain launch forms it. */
enum CalcHoGemm {
  HO_HEADS,          /* the multi-head loss: k_ho_delta_heads */
  HO_PLANES,         /* split-K planes in ho_slab, summed by the optimiser launch that follows */
  HO_PLANES_PAIRED,  /* the same, launched together with the rest rows of the weight-delta GEMM */
  HO_PAIRED_SUMMED,  /* not deferred (accumulation, an all-reduce between the ranks): still one launch with the rest rows, summed after it */
  HO_SUMMED          /* its own GEMM and k_ho_delta_finalize */
};
struct HoGemmPlan {
  CalcHoGemm form;
  int nkt, ks;
};
static inline HoGemmPlan ramd_plan_ho_gemm(const RamdShape *sh, const RamdBuffers *b, const CalcPlan &p, int nrows,
                                           int accumulate, bool ranges, int range_stride, bool active, bool defer) {
  HoGemmPlan h = {};
  if (ranges_are_heads(b, ranges, range_stride, p.flags) && sh->output_size % b->mheads_alen == 0 &&
      sh->output_size / b->mheads_alen <= 64 && env_int("RECUR_AMD_HO_HEADS", 1)) {
    h.form = HO_HEADS;
    return h;
  }
  h.nkt = (nrows + BK - 1) / BK;
  h.ks = pick_ks(((sh->H + BM - 1) / BM) * ((sh->O + BN - 1) / BN), h.nkt, b->slab_floats, (size_t)sh->H * sh->O);
  const bool planes = defer && !accumulate && !ranges && b->ho_slab;
  if (planes)
    h.form = p.has_rest && !active && env_int("RECUR_AMD_PAIR_HO", 1) ? HO_PLANES_PAIRED : HO_PLANES;
  else
    h.form = p.has_rest && !active && b->ho_slab && env_int("RECUR_AMD_PAIR_HO", 1) ? HO_PAIRED_SUMMED : HO_SUMMED;
  if (h.form != HO_SUMMED && h.ks > 8) h.ks = 8;
  return h;
}

/* k_delta_dma: whole 128-row tiles by LDS-DMA, one workgroup per CU; the rows above them (the input rows of a text
 * net) inside the same launch, or by the generic kernel with its own K split. */
struct DmaPlan {
  int rows_core, tm, tn, kd, blocks;
  int rest_rows;
  size_t rest_plane;
  bool rest_in;
  bool halves; /* the two-halves form (ramd_set_delta_half_hook) */
  int tmh, kd2, blocks2;
  int ks_rest;      /* planes of the rest rows, rest_off floats into the workspace, rest_plane apart */
  size_t rest_off;
};
/* ho_ready: the top layer's sums will be complete by the second half (an owed GEMM that is summed here, or the chain
 * launch has written ho_delta itself) */
static inline DmaPlan ramd_plan_delta_dma(const RamdShape *sh, const CalcPlan &p, bool ranges, bool defer, bool half_hook,
                                          bool ho_ready) {
  DmaPlan d = {};
  d.rows_core = (sh->I / 128) * 128;
  d.tm = d.rows_core / 128;
  d.tn = sh->hidden_size / 128;
  const int tiles = d.tm * d.tn;
  d.kd = 8;
  while (d.kd > 1 && tiles * d.kd > 256) d.kd >>= 1;
  while (d.kd > 1 && (d.kd > p.nkt || (size_t)d.kd * p.n > p.slab_floats)) d.kd >>= 1;
  const int per = 8 / d.kd;
  d.blocks = ((tiles + per - 1) / per) * 8;
  /* the rows above the last whole tile inside the same launch (see DeltaRest) when there are at
   * most 128 of them, at least four row tiles to share them out, and room for ks * tm planes */
  d.rest_rows = sh->I - d.rows_core;
  d.rest_plane = (size_t)d.rest_rows * sh->H;
  d.rest_in = d.rest_rows > 0 && d.rest_rows <= 128 && d.tm >= 4 && d.kd * d.tm <= RAMD_MAX_REST_PLANES &&
              (size_t)d.kd * p.n + (size_t)d.kd * d.tm * d.rest_plane <= p.slab_floats && env_int("RECUR_AMD_DELTA_REST_IN", 1);
  d.rest_off = (size_t)d.kd * p.n;
  /* ---- the two-halves form: rows [0, tm / 2 tiles) with twice the K split (the same number of workgroups and of
   * slab bytes), summed into ih_delta, hook; then the upper tiles with the rest rows riding along, the top layer's
   * deltas, summed, hook */
  /* OFF by default -- measured with ONE rank (bench.py --dist, round 3): 305 against 255 us per
   * generation.  Two launches of half the rows with twice the K split cost the GEMM class +24 us
   * (each workgroup's prologue, epilogue and ring fill amortise over 20 instead of 40 K tiles, the
   * finalize sums 8 planes twice), the two event hand-overs and RCCL calls another ~25 us: more
   * than the ~2.2 MB all-reduce it could hide is expected to take over xGMI.  And while a half's
   * GEMM holds every CU with 148 KB of LDS, RCCL's own workgroups can only become resident as that
   * launch drains.  Kept for the day a multi-GPU node says otherwise (RECUR_AMD_DIST_OVERLAP=1;
   * results equal the one-launch form: tests/test_gpu_dist.py). */
  d.halves = half_hook && !defer && d.rest_in && d.tm >= 8 && d.tm % 2 == 0 && ho_ready && !ranges &&
             env_int("RECUR_AMD_DIST_OVERLAP", 0);
  if (d.halves) {
    d.tmh = d.tm / 2;
    d.kd2 = 8;
    while (d.kd2 > 1 && (d.tmh * d.tn * d.kd2 > 256 || d.kd2 > p.nkt ||
                         (size_t)d.kd2 * p.n + (size_t)d.kd2 * d.tmh * d.rest_plane > p.slab_floats))
      d.kd2 >>= 1;
    const int per2 = 8 / d.kd2;
    d.blocks2 = ((d.tmh * d.tn + per2 - 1) / per2) * 8;
    d.rest_off = (size_t)d.kd2 * p.n;
  } else if (d.rest_in) {
    d.ks_rest = d.kd * d.tm;
  } else if (d.rest_rows > 0) {
    /* The rest rows' planes are compact ([ks_rest][I - rows_core][H], behind the core planes).
     * This GEMM is a few rows tall and K = S * D deep; measured at the north star its time does
     * not fall below 17 us for any K split from 16 to 48 (one workgroup per CU and ten K tiles
     * each, or three per CU and three tiles each: 0.87 us per 64 x 64 x 32 tile step and CU
     * either way), while every further plane costs the optimiser's sum: 16 it is. */
    d.ks_rest = pick_ks(((d.rest_rows + BM - 1) / BM) * ((sh->hidden_size + BN - 1) / BN), p.nkt, (size_t)RAMD_MAX_REST_PLANES, 1);
    if (d.ks_rest > RAMD_MAX_REST_PLANES) d.ks_rest = RAMD_MAX_REST_PLANES;
    if (d.ks_rest > p.nkt) d.ks_rest = p.nkt;
    while (d.ks_rest > 1 && (size_t)d.kd * p.n + (size_t)d.ks_rest * d.rest_plane > p.slab_floats) d.ks_rest--;
    if (d.ks_rest < 1) d.ks_rest = 1;
  }
  return d;
}
