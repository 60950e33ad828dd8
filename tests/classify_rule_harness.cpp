/* classify_rule_harness.cpp -- prints what recur_amd/csrc/classify_rule.h answers (tests/test_classify_rule.py): built with
 * the host compiler alone, no HIP; the same program runs under the sanitizers.
 *
 *   classify_rule_harness rows WIDTH LEN,LEN,... SKIP,SKIP,... CLASS,CLASS,...
 *       the batch laid over state rows as rnn_amd_classify_texts lays it -- texts_plan.h handed every length plus one --
 *       and walked launch by launch as its host loop walks a wave.  Per text k (the caller's order), lines
 *         fed<k>=t,t,...      the steps at which the plan has the text's row among the running prefix
 *         scored<k>=t,...     of those, the steps classify_skip_passed lets through
 *         counted<k>=t,...    of those, the steps whose class byte (CLASS[(k + t) % n_classes]) classify_has_class lets through
 *         rule<k>=f,s,c       how many t in [-2, len + 2] classify_fed, classify_scored and classify_counted say yes to;
 *       the program returns 3 where those functions and the walk disagree at any t.
 *   classify_rule_harness class OUTPUTS
 *       ok=...  the class bytes 0 .. 255 that classify_class_ok accepts for OUTPUTS outputs
 *       has=... those that classify_has_class says carry a class
 *   classify_rule_harness finish IGNORE_START LEN:SUM:SUMSQ ...
 *       per triple a line  n mean stddev  (%d %.17g %.17g): classify_scored_count and classify_finish */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <vector>
#include "classify_rule.h"
#include "texts_plan.h"

static std::vector<int> parse_list(const char *s) {
  std::vector<int> out;
  while (*s) {
    out.push_back((int)strtol(s, (char **)&s, 10));
    if (*s == ',') s++;
  }
  return out;
}

static void print_set(const char *name, int k, const std::set<int> &v) {
  printf("%s%d=", name, k);
  bool first = true;
  for (int t : v) {
    printf("%s%d", first ? "" : ",", t);
    first = false;
  }
  printf("\n");
}

static int rows(int width, const std::vector<int> &lens, const std::vector<int> &skips, const std::vector<int> &cls) {
  const int n = (int)lens.size();
  if ((int)skips.size() != n || cls.empty()) return 2;
  std::vector<int> lens1(n);
  for (int k = 0; k < n; k++) lens1[k] = lens[k] + 1; /* a text of len symbols has len forward passes */
  TextsPlan p;
  if (texts_plan_make(&p, lens1.data(), skips.data(), n, width)) return 1;
  std::vector<std::set<int>> fed(n), scored(n), counted(n);
  for (int w = 0; w < p.n_waves; w++) {
    const TextsWave *wave = &p.waves[w];
    int a_feed = 0;
    for (int t = 0; t <= wave->steps; t++) { /* the host loop of a wave: launch t scores step t - 1 and feeds step t */
      const int a_score = a_feed, t_score = t - 1;
      a_feed = t < wave->steps ? texts_plan_active(&p, w, t) : 0;
      for (int j = 0; j < a_feed; j++) fed[p.order[wave->row0 + j]].insert(t);
      for (int j = 0; j < a_score; j++) {
        const int k = p.order[wave->row0 + j];
        if (!classify_skip_passed(p.skip[wave->row0 + j], t_score)) continue;
        scored[k].insert(t_score);
        if (classify_has_class(cls[(size_t)(k + t_score) % cls.size()])) counted[k].insert(t_score);
      }
    }
  }
  texts_plan_free(&p);
  int bad = 0;
  for (int k = 0; k < n; k++) {
    print_set("fed", k, fed[k]);
    print_set("scored", k, scored[k]);
    print_set("counted", k, counted[k]);
    int f = 0, s = 0, c = 0;
    for (int t = -2; t <= lens[k] + 2; t++) {
      const int cl = cls[(size_t)(k + (t < 0 ? 0 : t)) % cls.size()];
      const int is_f = classify_fed(lens[k], t), is_s = classify_scored(lens[k], skips[k], t);
      const int is_c = classify_counted(lens[k], skips[k], t, cl);
      f += is_f, s += is_s, c += is_c;
      bad |= is_f != (int)fed[k].count(t) || is_s != (int)scored[k].count(t) || is_c != (int)counted[k].count(t);
    }
    printf("rule%d=%d,%d,%d\n", k, f, s, c);
  }
  return bad ? 3 : 0;
}

int main(int argc, char **argv) {
  if (argc >= 6 && !strcmp(argv[1], "rows"))
    return rows(atoi(argv[2]), parse_list(argv[3]), parse_list(argv[4]), parse_list(argv[5]));
  if (argc == 3 && !strcmp(argv[1], "class")) {
    std::set<int> ok, has;
    for (int b = 0; b < 256; b++) {
      if (classify_class_ok(b, atoi(argv[2]))) ok.insert(b);
      if (classify_has_class(b)) has.insert(b);
    }
    printf("ok=");
    for (int b : ok) printf("%d,", b);
    printf("\nhas=");
    for (int b : has) printf("%d,", b);
    printf("\n");
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "finish")) {
    const int ignore_start = atoi(argv[2]);
    for (int i = 3; i < argc; i++) {
      int len;
      double sum, sumsq, mean = -1.0, stddev = -1.0;
      if (sscanf(argv[i], "%d:%lf:%lf", &len, &sum, &sumsq) != 3) return 2;
      const int n = classify_scored_count(len, ignore_start);
      classify_finish(sum, sumsq, n, &mean, &stddev);
      printf("%d %.17g %.17g\n", n, mean, stddev);
    }
    return 0;
  }
  return 2;
}
