/* noise_ahead.c -- the presynaptic noise of a set's NEXT forward pass, generated now on a second stream (gnu11 C).
 *
 * A stream's generator is a sequential recurrence -- 3 x (h_size - 1) dependent steps per pass, one lane per stream,
 * 0.2 ms for 1028 values whatever the number of streams -- so the only way to take it off the generation's critical path
 * is to run it beside something else: it is launched as soon as the last draw before the next pass has been made (the
 * multi-head loss's leak decisions, or the pass itself in the text step) and runs beside the whole backward pass.  In
 * the multi-head step it is launched earlier still, between the pass and the loss: the generator is started from the
 * states the pass adopted, the loss's leak decisions on (one draw per head other than the stream's own, whatever the
 * outcome), beside the output layer and the loss instead of after them -- at 1024 / 256 / 73 x 50 the generator (0.31 ms
 * beside the matrix kernels) had become the generation's critical path.  The launch reads generator states and leaves
 * them alone; the forward pass adds the values and adopts the states that go with them (k_noise_apply, or inside
 * k_fwd_finalize_fused).
 *
 * WHETHER a pass may do that, and what an offer launches into which slot from where, is noise_ahead.h's, asked on
 * RamdEngine.ahead.  Here is the host's share and all of it: the side stream, the slots' device buffers, the events and
 * the launches (set_api.c, set_loss.c and set_train.c have the call sites, engine.c the two releases). */
#define RAMD_HIP_HOST 1
#include "rnn_host.h"

hipStream_t ramd_side_stream = NULL;

/* RECUR_AMD_NOISE_AHEAD: 0 off, 1 one pass ahead only, otherwise (and unset) two */
static int ahead_mode(void) {
  static int mode = -1;
  if (mode < 0) {
    const char *env = getenv("RECUR_AMD_NOISE_AHEAD");
    mode = !env ? 2 : atoi(env) == 0 ? 0 : atoi(env) == 1 ? 1 : 2;
  }
  return mode;
}

/* the side stream, made at its first use (dream_api.c draws a frame's noise ahead on it as well) */
hipStream_t ramd_side_stream_ensure(void) {
  if (!ramd_side_stream) {
    HIP_OK(hipStreamCreateWithFlags(&ramd_side_stream, hipStreamNonBlocking));
    ramd_note_side_stream();
  }
  return ramd_side_stream;
}

static void ahead_ensure_device(RamdEngine *e) {
  RamdNoiseAheadDev *d = &e->ahead_dev;
  ramd_side_stream_ensure();
  if (!d->go) {
    HIP_OK(hipEventCreateWithFlags((hipEvent_t *)&d->go, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags((hipEvent_t *)&d->done[0], hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags((hipEvent_t *)&d->done[1], hipEventDisableTiming));
  }
  for (int k = 0; k < 2; k++) {
    if (!d->noise[k]) {
      d->noise[k] = ramd_dev_alloc((size_t)e->sh.Scap * e->sh.H * sizeof(float));
      d->states[k] = ramd_dev_alloc((size_t)e->sh.Scap * sizeof(rand_ctx));
    }
  }
}

void ramd_noise_ahead_offer(RnnAmdSet *set, int loss_classes) {
  RamdEngine *e = set->eng;
  RamdNoiseAheadDev *d = &e->ahead_dev;
  const float level = set->nets[0]->presynaptic_noise;
  if (e->sh.bI || set->fwd_only) {
    return;
  }
  const int r0 = set->row0;
  const NoiseAheadPlan plan = noise_ahead_offer(&e->ahead, r0, set->n, level, loss_classes, ahead_mode());
  if (!plan.n_launches) {
    return;
  }
  ahead_ensure_device(e);
  /* behind the main stream: the draws made so far, and the last reader of a slot filled again (the pass just made) */
  HIP_OK(hipEventRecord((hipEvent_t)d->go, ramd_stream));
  HIP_OK(hipStreamWaitEvent(ramd_side_stream, (hipEvent_t)d->go, 0));
  for (int i = 0; i < plan.n_launches; i++) {
    const NoiseAheadLaunch *l = &plan.launch[i];
    ramd_launch_noise_speculate(ramd_side_stream, &e->sh, &e->b, r0, set->n, level, d->noise[l->dst], d->states[l->dst],
                                l->src == NOISE_AHEAD_GENERATORS ? NULL : d->states[l->src],
                                l->n_classes ? e->d_mclass + r0 : NULL, l->n_classes, l->skip);
    HIP_OK(hipEventRecord((hipEvent_t)d->done[l->dst], ramd_side_stream));
  }
}

void ramd_noise_ahead_pass(RamdEngine *e, int r0, int n, float level) {
  const RamdNoiseAheadDev *d = &e->ahead_dev;
  const int k = noise_ahead_pass(&e->ahead, r0, n, level, e->sh.bI != 0);
  if (k >= 0) {
    HIP_OK(hipStreamWaitEvent(ramd_stream, (hipEvent_t)d->done[k], 0));
    e->b.noise_spec = d->noise[k];
    e->b.rng_spec = d->states[k];
    e->b.noise_spec_use = 1;
  }
}

void ramd_noise_ahead_pass_done(RamdEngine *e) {
  e->b.noise_spec = NULL;
  e->b.rng_spec = NULL;
  e->b.noise_spec_use = 0;
}

int ramd_noise_ahead_adopted(const RamdEngine *e) { return e->ahead.adopted >= 0; }

void ramd_noise_ahead_free_device(RamdEngine *e) {
  RamdNoiseAheadDev *d = &e->ahead_dev;
  if ((e->ahead.slot[0].pending || e->ahead.slot[1].pending) && ramd_side_stream) {
    HIP_OK(hipStreamSynchronize(ramd_side_stream)); /* it writes into the buffers freed below */
  }
  noise_ahead_freed(&e->ahead);
  for (int k = 0; k < 2; k++) {
    ramd_dev_free(d->noise[k]);
    ramd_dev_free(d->states[k]);
    d->noise[k] = NULL;
    d->states[k] = NULL;
  }
  ramd_noise_ahead_pass_done(e);
}

void ramd_noise_ahead_destroy(RamdEngine *e) {
  RamdNoiseAheadDev *d = &e->ahead_dev;
  if (d->go) {
    HIP_OK(hipEventDestroy((hipEvent_t)d->go));
    HIP_OK(hipEventDestroy((hipEvent_t)d->done[0]));
    HIP_OK(hipEventDestroy((hipEvent_t)d->done[1]));
    d->go = d->done[0] = d->done[1] = NULL;
  }
}
