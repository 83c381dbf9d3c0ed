/*
 * host_pack_check.c -- rdsp_pack_runs (csrc/rdsp_pack_host.c, linked alone) as a program of its own, also for a build with
 * -fsanitize=address,undefined.  It reads cases from the file named on the command line (stdin without one); a case is
 *   first_block max_runs n_records          then n_records lines of          channel block
 * and for every case prints "runs N" (the return value; "refused CODE" for a negative one), then the runs written -- the first
 * min(N, max_runs) -- as "channel block n_blocks record" lines.  The record and run arrays are heap buffers of exactly
 * n_records and max_runs elements.  Prints "host_pack_check OK" at the end.
 */
#include <inttypes.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "rdsp.h"

static char g_err[512];
void rdsp_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
const char *rdsp_last_error(void) { return g_err; }

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
  int64_t first_block;
  int max_runs, n_records;
  while (fscanf(f, "%" SCNd64 " %d %d", &first_block, &max_runs, &n_records) == 3) {
    if (n_records < 0 || max_runs < 0) { fprintf(stderr, "bad case\n"); return 1; }
    rdsp_pack_record_t *rec = n_records ? (rdsp_pack_record_t *)malloc((size_t)n_records * sizeof *rec) : NULL;
    rdsp_pack_run_t *run = max_runs ? (rdsp_pack_run_t *)malloc((size_t)max_runs * sizeof *run) : NULL;
    for (int k = 0; k < n_records; k++)
      if (fscanf(f, "%" SCNd32 " %" SCNd32, &rec[k].channel, &rec[k].block) != 2) { fprintf(stderr, "short case\n"); return 1; }
    const int n = rdsp_pack_runs(rec, n_records, first_block, run, max_runs);
    if (n < 0) printf("refused %d\n", n);
    else {
      printf("runs %d\n", n);
      for (int k = 0; k < n && k < max_runs; k++)
        printf("%" PRId32 " %" PRId64 " %" PRId32 " %" PRId32 "\n", run[k].channel, run[k].block, run[k].n_blocks, run[k].record);
    }
    free(rec);
    free(run);
  }
  if (f != stdin) fclose(f);
  printf("host_pack_check OK\n");
  return 0;
}
