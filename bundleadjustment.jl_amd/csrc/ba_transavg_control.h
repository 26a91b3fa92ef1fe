// Host-only: the scalar decisions of ba_average_translations' Levenberg-Marquardt loop (include/ba_hip.h, "translation
// averaging").  No HIP in here.  ba_transavg_kernels.hip feeds it the two costs of every trial; ba_transavg_lm_decide
// exports it so that tests/test_translation_averaging.py can drive it on scripted cost sequences without a device.
#pragma once
#include <algorithm>
#include <cmath>

constexpr double TA_LAMBDA_MIN = 1e-9, TA_LAMBDA_MAX = 1e8;
enum { TA_GO = 0, TA_STOP_FTOL = 1, TA_STOP_LAMBDA = 2, TA_STOP_ITERATIONS = 3 };

struct TransavgDecision {
  int accepted;   // the trial replaces the iterate: F_trial < F (a NaN trial is rejected)
  int stop;       // TA_*
  double lambda;  // the damping of the next solve
};

// After the trial of iteration `iteration` (1-based) under `lambda`: F the cost of the iterate, F_trial that of the trial.
//   accepted iff F_trial < F; lambda <- max(lambda / 3, 1e-9) on acceptance, 4 lambda otherwise.
//   stop, the first that holds: |F - F_trial| <= ftol F (the change, either way, is below the tolerance: a rejected trial that
//   raises F by rounding alone ends the solve like an accepted one that lowers it by as little); the new lambda > 1e8;
//   iteration >= max_iterations.
inline TransavgDecision transavg_lm_decide(double F, double F_trial, double lambda, int iteration, int max_iterations, double ftol) {
  TransavgDecision d;
  d.accepted = F_trial < F ? 1 : 0;
  d.lambda = d.accepted ? std::max(lambda / 3.0, TA_LAMBDA_MIN) : 4.0 * lambda;
  d.stop = TA_GO;
  if (std::fabs(F - F_trial) <= ftol * F) d.stop = TA_STOP_FTOL;
  else if (d.lambda > TA_LAMBDA_MAX) d.stop = TA_STOP_LAMBDA;
  else if (iteration >= max_iterations) d.stop = TA_STOP_ITERATIONS;
  return d;
}
