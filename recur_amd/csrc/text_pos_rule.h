/* text_pos_rule.h -- where stream j of a training set reads the text at position i of an epoch
 * (charmodel-predict.c:273, 295-298), stated once: for k_assemble, k_bottom_forward (k_fwd_stages.h) and fwd_fused_tile
 * (k_fwd_fused.h), for the per-net loop of char_epoch.c, and for any host compiler alone (tests/text_pos_rule_harness.cpp).
 * No HIP header is needed: under hipcc a host and device function, elsewhere a plain inline one.  Plain C and valid C++.
 * The streams of a set of `global_count` start `spacing = (len - 1) / global_count` symbols apart and wrap at len - 1, so
 * that the target, the byte after the symbol, is always inside the text.  The reference writes
 * (i + stream * spacing) % (len - 1); here it is one conditional subtraction, which is the same number under the
 * PRECONDITION  0 <= i <= len - 1  and  0 <= stream < global_count  (what ramd_set_check_text_pos admits, and a set's own
 * stream numbers): stream * spacing <= len - 1 - spacing.  Nothing divides by len - 1: a text of one byte gives offset 0. */
#ifndef RAMD_TEXT_POS_RULE_H
#define RAMD_TEXT_POS_RULE_H 1

#ifndef RAMD_HD /* (sample_rule.h's, where that came first) */
#if defined(__HIP__) || defined(__HIPCC__)
#define RAMD_HD __attribute__((host)) __attribute__((device)) inline
#else
#define RAMD_HD static inline
#endif
#endif

/* the offset of the stream's symbol; its target is text[offset + 1].  `stream`: the stream's number among the
 * global_count of the whole set (a shard's first stream is not 0) */
RAMD_HD int text_pos(int len, int global_count, int stream, int i) {
  const int last = len - 1, spacing = last / global_count;
  int o = i + stream * spacing;
  if (o >= last) o -= last;
  return o;
}

#endif
