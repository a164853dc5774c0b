/*
 * mfe_exact.c — TEST INFRASTRUCTURE ONLY (see oracle/README.md).
 *
 * NOT the reference, which has no maximum-score folding.  The inside loops of
 * mccaskill_oracle.c compiled a third time, with Score = double (ORACLE_EXACT) and logsumexp
 * replaced by max (ORACLE_MAXPLUS, oracle_scoring.h).  The inside recurrences use only + and
 * logsumexp, so under (max, +) every sum over structures becomes the maximum over the same
 * structures: sums_external[0][n-1] is the score of the best structure of the model's space,
 * loop scores evaluated in f64.  No traceback: it checks the value that the HIP sweep
 * (rnamc_mfe.hip) and its traceback must reach, at any length the cubic loops can afford.
 */
#define ORACLE_EXACT 1
#define ORACLE_MAXPLUS 1
#include "mccaskill_oracle.c"

/* *best: the maximum score; mask: n x n row-major, 0 = the pair may not close, or NULL */
int rnamc_oracle_mfe_exact(const rnamc_params* p, const uint8_t* seq, uint32_t n,
                           int uses_contra_model, int allows_short_hairpins, const uint8_t* mask,
                           double* best) {
  int st = check_args(p, seq, n);
  if (st) return st;
  if (!best) return RNAMC_ERR_INVALID_ARG;
  ostate s;
  st = ostate_init(&s, n);
  if (st) return st;
  s.mask = mask;
  if (uses_contra_model)
    o_get_fold_sums_contra(p, seq, &s, allows_short_hairpins);
  else
    o_get_fold_sums(p, seq, &s);
  *best = s.sums_external[IDX(0, n - 1)];
  ostate_free(&s);
  return RNAMC_OK;
}
