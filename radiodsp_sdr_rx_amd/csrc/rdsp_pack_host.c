/*
 * rdsp_pack_host.c -- the host-only helper of rdsp_engine_pack_active (include/rdsp.h): rdsp_pack_runs merges a pack's
 * records into runs of consecutive blocks of one receiver.  Plain C, no device code; tests/host/host_pack_check.c links this
 * file alone.
 */
#include "rdsp_host.h"

int rdsp_pack_runs(const rdsp_pack_record_t *records, int n_records, int64_t first_block, rdsp_pack_run_t *runs, int max_runs) {
  if (n_records < 0 || max_runs < 0 || (n_records > 0 && !records) || (max_runs > 0 && !runs) || first_block > INT64_MAX - INT32_MAX) {
    rdsp_set_error("rdsp_pack_runs: bad argument (n_records %d and max_runs %d not negative, their arrays not NULL, first_block + block an int64)",
                   n_records, max_runs);
    return RDSP_ERR_INVALID;
  }
  for (int k = 0; k < n_records; k++) { /* everything is checked before anything is written */
    const rdsp_pack_record_t r = records[k];
    const int ascending = k == 0 || records[k - 1].channel < r.channel || (records[k - 1].channel == r.channel && records[k - 1].block < r.block);
    if (r.channel < 0 || r.block < 0 || !ascending) {
      rdsp_set_error("rdsp_pack_runs: record %d {channel %d, block %d} is negative or not above the record in front of it", k, (int)r.channel, (int)r.block);
      return RDSP_ERR_INVALID;
    }
  }
  int n = 0;
  for (int k = 0; k < n_records; k++) {
    const rdsp_pack_record_t r = records[k];
    if (k > 0 && records[k - 1].channel == r.channel && records[k - 1].block + 1 == r.block) {
      if (n <= max_runs) runs[n - 1].n_blocks++;
      continue;
    }
    if (n < max_runs) {
      runs[n].channel = r.channel; runs[n].n_blocks = 1; runs[n].record = k;
      runs[n].block = first_block + (int64_t)r.block;
    }
    n++;
  }
  return n;
}
