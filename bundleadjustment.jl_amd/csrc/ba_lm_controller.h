// The scalar side of ba_lm_solve: from the sums the device publishes to accept / reject, the next lambda, the stopping
// tests, the log row and the final status.  Host only (standard headers and the public header): the device loop of
// ba_lm.hip drives it, tests/test_lm_controller.py drives it on the CPU with a numpy step.
// variant 1 follows src/lm.jl:15-418, variant 0 src/LevenbergMarquardt.jl:16-385.
#pragma once
#include <cmath>

#include "../../include/ba_hip.h"

// A scalar with the width Julia's promotion rules give it: an operation rounds to Float32 exactly when both operands are
// Float32 (Base promotion: Float32 op Float64 -> Float64).  Used by ba_lm_solve for Float32 models.
namespace ts {
struct TS {
  double v;
  int w;  // 32 | 64
};
static inline TS f32(double x) { return TS{(double)(float)x, 32}; }
static inline TS f64(double x) { return TS{x, 64}; }
static inline bool both32(TS a, TS b) { return a.w == 32 && b.w == 32; }
static inline TS add(TS a, TS b) { return both32(a, b) ? f32((float)a.v + (float)b.v) : f64(a.v + b.v); }
static inline TS sub(TS a, TS b) { return both32(a, b) ? f32((float)a.v - (float)b.v) : f64(a.v - b.v); }
static inline TS mul(TS a, TS b) { return both32(a, b) ? f32((float)a.v * (float)b.v) : f64(a.v * b.v); }
static inline TS div(TS a, TS b) { return both32(a, b) ? f32((float)a.v / (float)b.v) : f64(a.v / b.v); }
static inline TS max(TS a, TS b) { return TS{a.v > b.v ? a.v : b.v, both32(a, b) ? 32 : 64}; }
static inline TS sqrt(TS a) { return a.w == 32 ? f32(std::sqrt((float)a.v)) : f64(std::sqrt(a.v)); }
// x^n with a variable Int n (lm.jl:308,331).  The reference ran on Julia 1.3 / 1.4 (.travis.yml:6-9), whose
// ^(x::Float64, y::Integer) and ^(x::Float32, y::Integer) are llvm.pow of the exponent CONVERTED to the base's type
// (base/math.jl there; power_by_squaring is the generic fallback for other number types and only became the float path in
// Julia 1.8's pow_body): pow() / powf() of the rounded exponent is that operation.
static inline TS powi(TS a, int n) { return a.w == 32 ? f32(std::pow((float)a.v, (float)n)) : f64(std::pow(a.v, (double)n)); }
}  // namespace ts

// The sums of squares one linearisation and one trial step publish (all ranks' contributions added).  Robust loss: rsq and
// rsq_trial hold 2 f instead of |r|^2, rtsq |r~|^2.
struct LMSums {
  double rsq;        // |r|^2 at x
  double rtsq;       // |r~|^2 at x (robust loss only)
  double gsq;        // |J'r|^2 at x
  double xsq;        // |x|^2
  double model;      // |J delta + c_r r|^2
  double rsq_trial;  // |r|^2 at x + delta
  double deltasq;    // |delta|^2
};

// one log row, the reference's columns (src/lm.jl:120-121,304): rho is ared / pred, in variant 0 1/2 |delta_r|^2
struct LMRow {
  int iter;
  double f, df, norm_jtr, lambda, norm_delta, rho;
  int accepted;
};

// One solve's scalars.  The calls of an iteration, in order:
//   begin_iteration, judge, { wants_halving, halve, judge }*, step_norm, reject | accept [, refreshed], end_iteration.
//
// Scalars carry the width Julia's promotion rules give them (TS: value + 32 | 64).  For a Float64 model everything is
// a Float64 and the arithmetic is plain double arithmetic.  For eltype(x) = Float32 (src/lm.jl:20-26,36-59):
// norm() of a Float32 vector, obj = norm_r^2 / 2, pred, ared, rho are Float32; the eps(Float32)-derived default
// tolerances and nu_d, nu_m, delta_d, lambda are Float32 VALUES whose expressions run in Float32, while a value the
// caller passes is a Float64 (the reference's own Float32 experiment passes Float64 literals, src/diffprecsions.jl:22) and
// promotes its expression; lambda = T(max(lambda, 1e10 / norm_Jtr)) (lm.jl:59) stays a Float32 until the first accepted
// step, whose `max(1.0e-8, lambda)` (lm.jl:337, a Float64 literal) makes it a Float64 for the rest of the run; in
// LevenbergMarquardt.jl only Float32 operations touch it.  The accept tests multiply by Float64 literals (lm.jl:259,335).
// (hidden: the members the compiler does not inline must not become exports of the library that includes this)
class __attribute__((visibility("hidden"))) LMController {
 public:
  using TS = ts::TS;
  // the resolved options (defaults: src/lm.jl:20-26 / src/LevenbergMarquardt.jl:21-26)
  TS restol, satol, srtol, oatol, ortol, atol, rtol, nu_d, nu_m, delta_d;
  int ite_max;

  // robust: a loss other than the linear one is set (Float64 models only): obj = f and norm_r = sqrt(2 f) enter the stopping
  // tests as they are; pred = 1/2 |r~|^2 - 1/2 |J~ delta + r~|^2 and the model value dr2 = f - pred.
  // cr0: the c_r of a fresh step, delta_r = -(J delta + c_r r)   (1; 1/mu in the Float16 branch)
  LMController(const ba_lm_opts &o, bool robust, double cr0)
      : V(o.variant), xf32(o.x_f32 != 0), robust(robust), linesearch(V && o.linesearch), facto_qr(o.facto >= 1),
        normalize_a(o.normalize == 2), cr0(cr0) {
    const TS eps = T_(xf32 ? 1.1920928955078125e-07 : 2.220446049250313e-16), sq = ts::sqrt(eps);
    const TS cbr = T_(std::pow(eps.v, 1.0 / 3.0));  // eltype(x)(eps^(1/3)): a Float64 power, converted
    const TS c100 = ts::mul(T_(100), sq), c1000 = ts::mul(T_(1000), sq);
    auto opt = [](double given, TS dflt, bool positive) { return (positive ? given > 0 : given >= 0) ? ts::f64(given) : dflt; };
    restol = opt(o.restol, V ? cbr : c100, false), satol = opt(o.satol, sq, false), srtol = opt(o.srtol, sq, false);
    oatol = opt(o.oatol, sq, false), ortol = opt(o.ortol, V ? cbr : c1000, false);
    atol = opt(o.atol, V ? sq : c100, false), rtol = opt(o.rtol, V ? cbr : c1000, false);
    nu_d = opt(o.nu_d, T_(3), true), nu_m = opt(o.nu_m, T_(3), true), delta_d = opt(o.delta_d, T_(2), true);
    lam = opt(o.lambda, T_(V ? 30 : 0.1), true);
    ite_max = o.ite_max >= 0 ? o.ite_max : (V ? 200 : 100);
    norm_delta = dr2 = ared = pred = nd = T_(0);
  }

  // the first linearisation (lm.jl:39-59,107-115).  all_fixed: every parameter is fixed (ba_lm_set_fixed): nothing to solve
  // for -- status :first_order, iter 0, before anything divides 0 by 0
  void start(const LMSums &s, bool all_fixed) {
    norm_r = norm_of(s.rsq, W());
    obj = robust ? half_of(s.rsq) : ts::div(ts::mul(norm_r, norm_r), T_(2));
    norm_Jtr = norm_of(s.gsq, W());
    norm_x = norm_of(s.xsq, W());
    if (all_fixed) norm_Jtr = T_(0);
    if (V && !all_fixed) {  // lm.jl:59: lambda = T(max(lambda, 1e10 / norm_Jtr))
      lam = ts::max(lam, ts::div(ts::f64(1e10), norm_Jtr));
      lam = T_(lam.v);
    }
    eps_first = ts::add(atol, ts::mul(rtol, norm_Jtr));  // lm.jl:107
    old_obj = obj;
    first_order = all_fixed || norm_Jtr.v < eps_first.v;
    small_residual = norm_r.v < restol.v;
    tired = iter_ > ite_max;
  }

  bool done() const { return small_step || first_order || small_residual || small_obj_change || tired || fail2; }

  void begin_iteration() {
    if (V) iter_++;  // lm.jl:127
    ntimes = 0;
    c_r_ = cr0;
    // the reference's delta is a Vector{Float32} for a Float32 model -- except under normalize = :A once lambda is a
    // Float64 (delta /= sqrt(lambda), lm.jl:235-237) or behind a Float64 delta_d in the line search (lm.jl:266)
    delta_w = (xf32 && !(V && normalize_a && lam.w == 64)) ? 32 : 64;
  }

  // the accept test on a trial step's sums: the first try of an iteration and each halved step of the line search
  void judge(const LMSums &s) {
    dr2 = half_of(s.model);  // 1/2 |delta_r|^2   (lm.jl:229)
    const TS pred_r = ts::f64(0.5 * s.rtsq - 0.5 * s.model);  // (robust loss only)
    if (robust) dr2 = ts::sub(obj, pred_r);
    obj_suiv = half_of(s.rsq_trial);
    norm_rsuiv = norm_of(s.rsq_trial, W());
    if (V) {
      pred = robust ? pred_r : ts::sub(obj, dr2);
      ared = ts::sub(obj, obj_suiv);
      accepted_ = ared.v >= 1e-4 * pred.v;  // lm.jl:257-259 (Float64 literal)
    } else {
      iter_++;  // LevenbergMarquardt.jl:240
      accepted_ = ts::sub(obj_suiv, obj).v < 1e-4 * (robust ? -pred_r.v : ts::sub(dr2, obj).v);  // LevenbergMarquardt.jl:243
    }
  }

  bool wants_halving() const { return linesearch && !accepted_ && ntimes < 4; }  // lm.jl:264-295

  struct Halving {
    double scale;  // delta *= scale
    double c_r;    // the model value of the scaled step is |J delta + c_r r|^2
  };
  // delta /= delta_d ; delta_r = (delta_r - r)/delta_d (lm.jl:277): with delta_r = -(J delta + c r) the update is
  // c <- (c + 1)/delta_d, which stays 1 only for the default delta_d = 2 (the reference's comment at lm.jl:275-276
  // assumes it; the code is followed, not the comment)
  // The :QR branch recomputes |J delta + r|^2 instead (lm.jl:273): c stays 1 there (:PCG has no dr vector to recur on
  // either: it re-evaluates like :QR).
  Halving halve() {
    if (!facto_qr) c_r_ = (c_r_ + 1.0) / delta_d.v;
    if (delta_d.w == 64) delta_w = 64;
    ntimes++;
    return Halving{1.0 / delta_d.v, c_r_};
  }

  // |delta| of the step just judged.  false: it is NaN (lm.jl:297-302) -- the run ends, status :exception
  bool step_norm(const LMSums &s) {
    nd = norm_of(s.deltasq, delta_w);
    if (!V) return true;
    norm_delta = nd;
    if (std::isnan(norm_delta.v)) fail2 = true;
    return !fail2;
  }

  bool accepted() const { return accepted_; }

  void reject() {
    if (V) lam = ts::mul(ts::max(lam, ts::div(norm_delta.w == 32 ? ts::f32(1) : ts::f64(1), norm_delta)), ts::powi(nu_m, ntimes + 1));  // lm.jl:308
    else lam = ts::mul(lam, nu_m);                                                            // LevenbergMarquardt.jl:269
  }

  // x .= x_suiv.  true: a stopping test that needs no new linearisation already holds (the refresh then goes out without the
  // next trial step)
  bool accept() {
    if (V) {  // lm.jl:329-337
      if (ntimes > 0) lam = ts::div(lam, ts::powi(nu_d, ntimes - 1));
      else lam = ts::div(lam, nu_d);
      if (ared.v >= 0.9 * pred.v) lam = ts::div(lam, nu_d);
      lam = ts::max(ts::f64(1.0e-8), lam);  // the Float64 literal promotes lambda for the rest of the run
    } else {
      lam = ts::div(lam, nu_d);  // LevenbergMarquardt.jl:292
    }
    old_obj = obj;
    norm_r = norm_rsuiv;
    obj = obj_suiv;
    return stopping_tests(nullptr) || iter_ > ite_max;
  }

  // J, J'r at the accepted point (lm.jl:341,370)
  void refreshed(const LMSums &s) {
    if (!V) norm_delta = nd;  // LevenbergMarquardt.jl:352
    stopping_tests(&s);
  }

  void end_iteration() { tired = iter_ > ite_max; }  // lm.jl:382

  // variant 1: the row of the step just judged, after step_norm (lm.jl:304).  variant 0: the state as an iteration begins and
  // as the run ends (LevenbergMarquardt.jl:143-147,368)
  LMRow row() const {
    const double df = ts::sub(old_obj, obj).v;
    if (V) return LMRow{iter_, obj.v, df, norm_Jtr.v, lam.v, norm_delta.v, ts::div(ared, pred).v, (accepted_ && dr2.v <= obj.v) ? 1 : 0};
    return LMRow{iter_, obj.v, df, norm_Jtr.v, lam.v, norm_delta.v, dr2.v, accepted_ ? 1 : 0};
  }

  int status() const {  // lm.jl:391-405
    if (small_step) return BA_ST_SMALL_STEP;
    if (first_order) return BA_ST_FIRST_ORDER;
    if (small_residual) return BA_ST_SMALL_RESIDUAL;
    if (small_obj_change) return BA_ST_ACCEPTABLE;
    if (fail2) return BA_ST_EXCEPTION;
    if (tired) return BA_ST_MAX_ITER;
    return BA_ST_UNKNOWN;
  }

  TS lambda_ts() const { return lam; }
  double lambda() const { return lam.v; }
  double c_r() const { return c_r_; }
  int iter() const { return iter_; }
  double objective() const { return obj.v; }
  double dual_feas() const { return norm_Jtr.v; }

 private:
  const int V;
  const bool xf32, robust, linesearch, facto_qr, normalize_a;
  const double cr0;
  TS lam, obj, old_obj, norm_r, norm_Jtr, norm_x, norm_delta, dr2, pred, ared, eps_first;
  TS obj_suiv, norm_rsuiv, nd;  // of the step being judged
  int iter_ = 0, ntimes = 0, delta_w = 64;
  double c_r_ = 1.0;
  bool small_step = false, first_order = false, small_residual = false, small_obj_change = false, tired = false, fail2 = false;
  bool accepted_ = false;

  int W() const { return xf32 ? 32 : 64; }
  TS T_(double v) const { return xf32 ? ts::f32(v) : ts::f64(v); }  // a value of type eltype(x)
  // norm(v) from the device's sum of squares; 1/2 |v|^2 the way the reference forms it (norm(v)^2 / 2: for a Float32
  // vector the norm is rounded to Float32 first; for Float64 the sum of squares is halved directly)
  static TS norm_of(double sumsq, int wd) { return wd == 32 ? ts::f32(std::sqrt(sumsq)) : ts::f64(std::sqrt(sumsq)); }
  TS half_of(double sumsq) const {
    if (!xf32) return ts::f64(0.5 * sumsq);
    const TS n = ts::f32(std::sqrt(sumsq));
    return ts::div(ts::mul(n, n), ts::f32(2));
  }
  // lm.jl:375-379.  s: the sums of the new linearisation; null before it, when only the tests that need neither |J'r| nor |x|
  // can be made.  Returns whether one of them holds.
  bool stopping_tests(const LMSums *s) {
    if (s) {
      norm_Jtr = norm_of(s->gsq, W());
      norm_x = norm_of(s->xsq, W());
      small_step = norm_delta.v < ts::add(satol, ts::mul(srtol, norm_x)).v;
      first_order = norm_Jtr.v < eps_first.v;
    }
    small_residual = norm_r.v < restol.v;
    small_obj_change = ts::sub(old_obj, obj).v < ts::add(oatol, ts::mul(ortol, old_obj)).v;
    return small_step || first_order || small_residual || small_obj_change;
  }
};
