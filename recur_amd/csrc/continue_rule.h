/* continue_rule.h -- what launch t of rnn_amd_continue_texts does for one row, stated once: for k_texts_continue
 * (kernels_rows.hip), which asks it per row, for the host loop around it (sample_api.c), which asks it of a wave's longest
 * row, and for any host compiler alone (tests/continue_rule_harness.cpp asks it under g++).  No HIP header is needed:
 * under hipcc the function is a host and device function, elsewhere a plain inline one.  Plain C and valid C++.
 *
 * A row has a prompt of plen >= 1 symbols and draws up to max_len >= 1.  Between two launches lies one forward pass of
 * the rows that were fed, so the row's launches are t = 0 .. plen + max_len - 1:
 *   t < plen                  feed prompt symbol t; nothing is drawn, the generator is not touched.  At t == 0 the hidden
 *                             values of the feed are the net's (hid0), later the row's own
 *   plen <= t < plen + max_len  the forward pass before this launch was fed prompt symbol plen - 1 or the pick of launch
 *                             t - 1: draw text index t - plen from its output row, and feed the pick -- unless the index
 *                             was the last, max_len - 1 (or the pick ended the row: the kernel's business, not the rule's)
 *   later                     nothing
 * So a row is fed after launch t exactly when t < plen + max_len - 1: texts_plan.h's `len - 1 > t` for
 * len = plen + max_len, which is why that plan's order and row counts serve this call as they are. */
#ifndef RAMD_CONTINUE_RULE_H
#define RAMD_CONTINUE_RULE_H 1

#ifndef RAMD_HD /* (sample_rule.h's, where that came first) */
#if defined(__HIP__) || defined(__HIPCC__)
#define RAMD_HD __attribute__((host)) __attribute__((device)) inline
#else
#define RAMD_HD static inline
#endif
#endif

#define CONTINUE_IDLE 0   /* nothing: the row's launches are over */
#define CONTINUE_PROMPT 1 /* feed prompt symbol `index` */
#define CONTINUE_DRAW 2   /* draw text index `index`, then feed the pick if `feeds` */

typedef struct ContinueStep {
  int what;    /* CONTINUE_* */
  int index;   /* into the prompt, or into the text */
  int feeds;   /* an input row is built in this launch (a row that is done is still not fed) */
  int on_hid0; /* ... from the net's hidden row instead of the row's own */
} ContinueStep;

RAMD_HD ContinueStep continue_step(int plen, int max_len, int t) {
  ContinueStep st = {CONTINUE_IDLE, 0, 0, 0};
  if (t < 0 || plen < 1 || max_len < 1) {
    return st;
  }
  if (t < plen) {
    st.what = CONTINUE_PROMPT;
    st.index = t;
    st.feeds = 1;
    st.on_hid0 = t == 0;
  } else if (t - plen < max_len) { /* (no plen + max_len: the difference cannot overflow) */
    st.what = CONTINUE_DRAW;
    st.index = t - plen;
    st.feeds = st.index < max_len - 1;
  }
  return st;
}

#endif
