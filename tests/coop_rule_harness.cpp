// Asks recur_amd/csrc/coop_rule.h about a residency probe's answer, a seat mode or a flag sequence and prints what it says
// as key=value lines (tests/test_coop_rule.py).  Host code only.
//   table arrived fail xcc,cu_key xcc,cu_key ...   the probe's workgroups in order (any number up to 256; the rest of the
//                                                  probe's arrays stays zero, as the device's memset leaves it)
//   mode table static_requested in_turn side_streams
//   seq value                                      against both limits
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "coop_rule.h"

int main(int argc, char **argv) {
  if (argc >= 4 && !strcmp(argv[1], "table")) {
    static CoopProbe p;
    static SeatTable t;
    p.arrived = (unsigned)strtoul(argv[2], nullptr, 0), p.fail = (unsigned)strtoul(argv[3], nullptr, 0);
    if (argc - 4 > COOP_WGS) return fprintf(stderr, "more than %d workgroups\n", (int)COOP_WGS), 2;
    for (int i = 4; i < argc; i++) {
      char *comma = nullptr;
      p.xcc[i - 4] = (unsigned)strtoul(argv[i], &comma, 0);
      if (*comma != ',') return fprintf(stderr, "bad pair %s\n", argv[i]), 2;
      p.cu_key[i - 4] = (unsigned)strtoul(comma + 1, nullptr, 0);
    }
    printf("resident=%d\nin_turn=%d\n", coop_resident(&p), coop_in_turn(&p));
    const int ok = coop_seat_table(&p, &t);
    printf("table=%d\n", ok);
    if (ok) /* only the named entries: everything else must be COOP_NO_SEAT, which `unnamed_ok` says */
      for (int x = 0; x < COOP_XCDS; x++) {
        int unnamed_ok = 1;
        printf("seats%d=", x);
        for (int k = 0; k < COOP_CU_KEYS; k++) {
          if (t.seat[x][k] < (unsigned)COOP_SEATS) printf("%d:%u ", k, t.seat[x][k]);
          else if (t.seat[x][k] != COOP_NO_SEAT) unnamed_ok = 0;
        }
        printf("\nunnamed_ok%d=%d\n", x, unnamed_ok);
      }
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "mode")) {
    printf("mode=%d\n", coop_seat_mode(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "seq")) {
    const unsigned seq = (unsigned)strtoul(argv[2], nullptr, 0);
    /* the launcher asks, then counts up: the flag values below belong to seq + 1 where seq does not start over */
    printf("chain_starts_over=%d\nfwd_top_starts_over=%d\n", coop_seq_starts_over(seq, COOP_CHAIN_SEQ_LIMIT),
           coop_seq_starts_over(seq, COOP_FWD_TOP_SEQ_LIMIT));
    printf("chain_limit=%u\nfwd_top_limit=%u\nchain_epoch=%u\n", COOP_CHAIN_SEQ_LIMIT, COOP_FWD_TOP_SEQ_LIMIT, COOP_CHAIN_EPOCH);
    printf("chain_largest_flag=%llu\nfwd_top_largest_flag=%llu\n",
           (unsigned long long)(seq + 1ull) * COOP_CHAIN_EPOCH + (COOP_CHAIN_EPOCH - 1u), (unsigned long long)seq + 1ull);
    printf("abort_codes=%d,%d,%d,%d\n", COOP_ABORT_CHAIN, COOP_ABORT_CHAIN_OFF_XCD, COOP_ABORT_XCHG_BARRIER, COOP_ABORT_FWD_TOP);
    return 0;
  }
  return fprintf(stderr, "usage: table ... | mode t s i x | seq n\n"), 2;
}
