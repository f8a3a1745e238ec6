// TEST INFRASTRUCTURE (oracle/ref_build only): a stand-in for the part of Ceres Solver's interface that the reference's
// spherical_bundle_adjuster.cpp names, so that the file compiles unchanged without Ceres.  Written for this project from Ceres'
// public documentation (Jet arithmetic as documented for ceres::Jet: f + g, f * g = (f.a g.a, f.a g.v + f.v g.a), f / g through
// 1 / g.a, scalar operands scale both parts, sqrt / sin / cos / exp by the chain rule); none of it is Ceres' text.
//
//   Jet<T, N>             dual number, T = double or long double
//   AutoDiffCostFunction  EVALUATES: the functor runs on Jet<double>, Jet<long double> and plain long double
//   Problem               RECORDS residual blocks (cost, loss, parameter pointers) and lower bounds; it solves nothing
//   HuberLoss             holds its delta
//   Solve, Solver         declared only: the minimiser is out of scope and never run
#pragma once
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

namespace ceres {

template <typename T, int N> struct Jet {
  T a;
  T v[N];
  Jet() : a(0) { for (int i = 0; i < N; ++i) v[i] = T(0); }
  Jet(double s) : a(s) { for (int i = 0; i < N; ++i) v[i] = T(0); }   // NOLINT: implicit, as in Ceres
  static Jet variable(T value, int k) { Jet r; r.a = value; r.v[k] = T(1); return r; }
};
#define SBA_JET template <typename T, int N> inline
SBA_JET Jet<T, N> operator-(const Jet<T, N>& f) { Jet<T, N> r; r.a = -f.a; for (int i = 0; i < N; ++i) r.v[i] = -f.v[i]; return r; }
SBA_JET Jet<T, N> operator+(const Jet<T, N>& f, const Jet<T, N>& g) { Jet<T, N> r; r.a = f.a + g.a; for (int i = 0; i < N; ++i) r.v[i] = f.v[i] + g.v[i]; return r; }
SBA_JET Jet<T, N> operator+(const Jet<T, N>& f, double s) { Jet<T, N> r = f; r.a = f.a + s; return r; }
SBA_JET Jet<T, N> operator+(double s, const Jet<T, N>& f) { Jet<T, N> r = f; r.a = s + f.a; return r; }
SBA_JET Jet<T, N> operator-(const Jet<T, N>& f, const Jet<T, N>& g) { Jet<T, N> r; r.a = f.a - g.a; for (int i = 0; i < N; ++i) r.v[i] = f.v[i] - g.v[i]; return r; }
SBA_JET Jet<T, N> operator-(const Jet<T, N>& f, double s) { Jet<T, N> r = f; r.a = f.a - s; return r; }
SBA_JET Jet<T, N> operator-(double s, const Jet<T, N>& f) { Jet<T, N> r; r.a = s - f.a; for (int i = 0; i < N; ++i) r.v[i] = -f.v[i]; return r; }
SBA_JET Jet<T, N> operator*(const Jet<T, N>& f, const Jet<T, N>& g) { Jet<T, N> r; r.a = f.a * g.a; for (int i = 0; i < N; ++i) r.v[i] = f.a * g.v[i] + f.v[i] * g.a; return r; }
SBA_JET Jet<T, N> operator*(const Jet<T, N>& f, double s) { Jet<T, N> r; r.a = f.a * s; for (int i = 0; i < N; ++i) r.v[i] = f.v[i] * s; return r; }
SBA_JET Jet<T, N> operator*(double s, const Jet<T, N>& f) { Jet<T, N> r; r.a = s * f.a; for (int i = 0; i < N; ++i) r.v[i] = s * f.v[i]; return r; }
SBA_JET Jet<T, N> operator/(const Jet<T, N>& f, const Jet<T, N>& g) {
  Jet<T, N> r;
  const T a_inverse = T(1.0) / g.a;
  r.a = f.a * a_inverse;
  for (int i = 0; i < N; ++i) r.v[i] = (f.v[i] - r.a * g.v[i]) * a_inverse;
  return r;
}
SBA_JET Jet<T, N> operator/(const Jet<T, N>& f, double s) { Jet<T, N> r; const T s_inverse = T(1.0) / s; r.a = f.a * s_inverse; for (int i = 0; i < N; ++i) r.v[i] = f.v[i] * s_inverse; return r; }
SBA_JET Jet<T, N> operator/(double s, const Jet<T, N>& g) { Jet<T, N> r; const T k = -s / (g.a * g.a); r.a = s / g.a; for (int i = 0; i < N; ++i) r.v[i] = g.v[i] * k; return r; }
SBA_JET bool operator>(const Jet<T, N>& f, const Jet<T, N>& g) { return f.a > g.a; }
SBA_JET bool operator<(const Jet<T, N>& f, const Jet<T, N>& g) { return f.a < g.a; }
SBA_JET bool operator>(const Jet<T, N>& f, double s) { return f.a > s; }
SBA_JET bool operator<(const Jet<T, N>& f, double s) { return f.a < s; }
SBA_JET Jet<T, N> sqrt(const Jet<T, N>& f) { Jet<T, N> r; r.a = std::sqrt(f.a); const T two_a_inverse = T(1.0) / (T(2.0) * r.a); for (int i = 0; i < N; ++i) r.v[i] = f.v[i] * two_a_inverse; return r; }
SBA_JET Jet<T, N> sin(const Jet<T, N>& f) { Jet<T, N> r; r.a = std::sin(f.a); const T c = std::cos(f.a); for (int i = 0; i < N; ++i) r.v[i] = c * f.v[i]; return r; }
SBA_JET Jet<T, N> cos(const Jet<T, N>& f) { Jet<T, N> r; r.a = std::cos(f.a); const T s = -std::sin(f.a); for (int i = 0; i < N; ++i) r.v[i] = s * f.v[i]; return r; }
SBA_JET Jet<T, N> exp(const Jet<T, N>& f) { Jet<T, N> r; r.a = std::exp(f.a); for (int i = 0; i < N; ++i) r.v[i] = r.a * f.v[i]; return r; }
#undef SBA_JET

enum LinearSolverType { DENSE_QR, ITERATIVE_SCHUR };
enum NumericDiffMethodType { CENTRAL, FORWARD };

class LossFunction {
 public:
  virtual ~LossFunction() {}
  virtual double standin_delta() const = 0;
};
class HuberLoss : public LossFunction {
 public:
  explicit HuberLoss(double a) : a_(a) {}
  double standin_delta() const override { return a_; }

 private:
  double a_;
};

// One residual block's cost: sizes, and evaluation in three arithmetics.  Jacobians are row-major, num_residuals x (sum of the
// parameter-block sizes), columns in the order of the blocks.
class CostFunction {
 public:
  virtual ~CostFunction() {}
  virtual int standin_num_residuals() const = 0;
  virtual std::vector<int> standin_block_sizes() const = 0;
  virtual void standin_evaluate(double const* const* params, double* res, double* jac) const = 0;
  virtual void standin_evaluate_ld(double const* const* params, long double* res, long double* jac) const = 0;
  virtual void standin_residuals_ld(double const* const* params, long double* res) const = 0;   // T = long double, no Jet
};

template <typename Functor, int kNumResiduals, int N0, int N1 = 0, int N2 = 0>
class AutoDiffCostFunction : public CostFunction {
 public:
  explicit AutoDiffCostFunction(Functor* f) : functor_(f) {}
  ~AutoDiffCostFunction() override { delete functor_; }
  int standin_num_residuals() const override { return kNumResiduals; }
  std::vector<int> standin_block_sizes() const override {
    std::vector<int> s{N0};
    if (N1) s.push_back(N1);
    if (N2) s.push_back(N2);
    return s;
  }
  void standin_evaluate(double const* const* params, double* res, double* jac) const override { run<double>(params, res, jac); }
  void standin_evaluate_ld(double const* const* params, long double* res, long double* jac) const override { run<long double>(params, res, jac); }
  void standin_residuals_ld(double const* const* params, long double* res) const override {
    long double p[kParams > 0 ? kParams : 1];
    int at = 0;
    const int sizes[3] = {N0, N1, N2};
    for (int b = 0; b < 3; ++b)
      for (int i = 0; i < sizes[b]; ++i) p[at++] = params[b][i];
    call(p, res);
  }

 private:
  enum { kParams = N0 + N1 + N2 };
  template <typename T> void call(const T* p, T* res) const {
    call3(p, res, std::integral_constant<int, (N2 > 0) ? 3 : ((N1 > 0) ? 2 : 1)>());   // by the number of parameter blocks
  }
  template <typename T> void call3(const T* p, T* res, std::integral_constant<int, 1>) const { (*functor_)(p, res); }
  template <typename T> void call3(const T* p, T* res, std::integral_constant<int, 2>) const { (*functor_)(p, p + N0, res); }
  template <typename T> void call3(const T* p, T* res, std::integral_constant<int, 3>) const { (*functor_)(p, p + N0, p + N0 + N1, res); }
  template <typename S> void run(double const* const* params, S* res, S* jac) const {
    typedef Jet<S, kParams> J;
    J p[kParams], r[kNumResiduals];
    int at = 0;
    const int sizes[3] = {N0, N1, N2};
    for (int b = 0; b < 3; ++b)
      for (int i = 0; i < sizes[b]; ++i, ++at) p[at] = J::variable(static_cast<S>(params[b][i]), at);
    call(p, r);
    for (int i = 0; i < kNumResiduals; ++i) {
      res[i] = r[i].a;
      for (int k = 0; k < kParams; ++k) jac[i * kParams + k] = r[i].v[k];
    }
  }
  Functor* functor_;
};

template <typename Functor, NumericDiffMethodType kMethod, int kNumResiduals, int N0, int N1 = 0, int N2 = 0>
class NumericDiffCostFunction;   // named by a using-declaration of the reference, never instantiated

class Problem {
 public:
  struct Block {
    CostFunction* cost;
    LossFunction* loss;   // null: no loss
    std::vector<double*> params;
  };
  struct LowerBound {
    double* values;
    int index;
    double bound;
  };
  ~Problem() {
    for (Block& b : blocks) { delete b.cost; delete b.loss; }
  }
  template <typename... P> void AddResidualBlock(CostFunction* cost, LossFunction* loss, P*... p) {
    blocks.push_back(Block{cost, loss, std::vector<double*>{p...}});
  }
  void SetParameterLowerBound(double* values, int index, double lower_bound) { lower.push_back(LowerBound{values, index, lower_bound}); }
  std::vector<Block> blocks;
  std::vector<LowerBound> lower;
};

// declared only (never run)
class Solver {
 public:
  struct Options {
    LinearSolverType linear_solver_type = DENSE_QR;
    int max_num_iterations = 50;
    bool minimizer_progress_to_stdout = false;
    int num_threads = 1;
  };
  struct Summary {
    std::string BriefReport() const;
    int num_threads_given = 0;
    int num_threads_used = 0;
  };
};
void Solve(const Solver::Options& options, Problem* problem, Solver::Summary* summary);

}  // namespace ceres
