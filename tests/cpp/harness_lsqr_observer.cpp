// harness_lsqr_observer.cpp -- LSQR with a user function (reference IterativeSolvers.h:450-456, called at :845-851)
// through ONE templated driver compiled on the plain host vector of oracle/template_driver.inc, where the template
// layer's generic loop is the reference's statement sequence, and on MI355::DeviceVector with the tagged device
// callables, where the solve keeps the fused kernels and the user function observes it (mi_lsqr_observed) -- each with
// the empty pack and with Args = {size_t, Vec} (a counter the user function increments, and a cache).  Per call the user
// function records  k, |x| (as handed), <x,x>, |rbar|, |Abar' rbar|, |Abar|, cond(Abar)
// (tests/test_gpu_lsqr_observer.py).  The operator is the tridiagonal (lo, di, up).  TEST INFRASTRUCTURE ONLY.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "Optimization/LinearAlgebra/IterativeSolvers.h"
#include "Optimization/MI355/Device.h"
#include "Optimization/Riemannian/GradientDescent.h"
#include "Optimization/Riemannian/TNLS.h"
#include "Optimization/Riemannian/TNT.h"

#define DRV(name) hlb_##name
#include "template_driver.inc"  // HostVec (and its drivers under the hlb_ prefix, unused here)

using Optimization::MI355::Context;
using Optimization::MI355::DeviceVector;
namespace MI355 = Optimization::MI355;

static thread_local std::string g_msg;
extern "C" const char *hl_last_error() { return g_msg.c_str(); }

namespace {

constexpr int kRecCols = 7;
constexpr size_t kNever = ~(size_t)0;

struct LsqrObsOut {  // plain data, mirrored by ctypes in the test
  size_t nrec;       // calls of the user function
  size_t counter;    // the pack's counter after the call (pack runs)
  size_t iterations;
  double xnorm;
  unsigned long long fused_lsqr_solves, generic_lsqr_solves;  // over the solve (device)
  size_t syncs;                                               // mi_ctx_sync_count over the solve (device)
  double seconds;                                             // wall time of the LSQR call, device drained (device)
};

inline void bump() {}
template <typename V>
inline void bump(size_t &calls, V &) {
  ++calls;
}

// the one driver: LSQR<Vec, Vec, double, Args...> with a user function that records, stops at `stop_at`, throws at
// `throw_at`
template <typename Vec, typename... Args>
Vec observed_lsqr(const LA::LinearOperator<Vec, Vec, Args...> &A, const LA::LinearOperator<Vec, Vec, Args...> &At,
                  const Vec &b, const LA::InnerProduct<Vec, double, Args...> &ip, size_t max_iterations, double lambda,
                  double btol, double Atol, double Delta, bool with_user_function, size_t stop_at, size_t throw_at, double *rec,
                  size_t rec_cap, LsqrObsOut *out, Args &...args) {
  out->nrec = 0;
  std::optional<LA::LSQRUserFunction<Vec, Vec, double, Args...>> uf = LA::LSQRUserFunction<Vec, Vec, double, Args...>(
      [&](size_t k, const LA::LinearOperator<Vec, Vec, Args...> &, const LA::LinearOperator<Vec, Vec, Args...> &,
          const Vec &, const Vec &x, double xnorm, double rbar_norm, double Arnorm, double Anorm, double Acond,
          Args &...a) {
        if (k == throw_at) throw std::runtime_error("the user function threw");
        bump(a...);
        if (rec && out->nrec < rec_cap) {
          double *row = rec + out->nrec * kRecCols;
          row[0] = (double)k;
          row[1] = xnorm;
          row[2] = x.dot(x);
          row[3] = rbar_norm;
          row[4] = Arnorm;
          row[5] = Anorm;
          row[6] = Acond;
        }
        out->nrec++;
        return k == stop_at;
      });
  if (!with_user_function) uf.reset();
  double xn = 0;
  size_t it = 0;
  // (Abar_cond_limit out of the way: the cases are told apart by btol / Atol / Delta / max_iterations)
  Vec x = LA::LSQR<Vec, Vec, double, Args...>(A, At, b, ip, ip, args..., xn, it, max_iterations, lambda, btol, Atol, 1e300,
                                              Delta, uf);
  out->xnorm = xn;
  out->iterations = it;
  return x;
}

HostVec tridiag(size_t n, const double *lo, const double *di, const double *up, const HostVec &v, bool transpose) {
  HostVec o(n);
  for (size_t i = 0; i < n; ++i) {
    double s = di[i] * v.d[i];
    // row i of A: lo[i] at column i-1, up[i] at column i+1; of A': up[i-1] at column i-1, lo[i+1] at column i+1
    if (i > 0) s += (transpose ? up[i - 1] : lo[i]) * v.d[i - 1];
    if (i + 1 < n) s += (transpose ? lo[i + 1] : up[i]) * v.d[i + 1];
    o.d[i] = s;
  }
  return o;
}

template <typename... Args>
HostVec host_run(size_t n, const double *lo, const double *di, const double *up, const double *b, size_t max_iterations,
                 double lambda, double btol, double Atol, double Delta, bool with_uf, size_t stop_at, size_t throw_at,
                 double *rec, size_t rec_cap, LsqrObsOut *out, Args &...args) {
  LA::LinearOperator<HostVec, HostVec, Args...> A = [&](const HostVec &v, Args &...) {
    return tridiag(n, lo, di, up, v, false);
  };
  LA::LinearOperator<HostVec, HostVec, Args...> At = [&](const HostVec &v, Args &...) {
    return tridiag(n, lo, di, up, v, true);
  };
  LA::InnerProduct<HostVec, double, Args...> ip = [](const HostVec &a, const HostVec &c, Args &...) { return a.dot(c); };
  return observed_lsqr<HostVec, Args...>(A, At, HostVec(b, n), ip, max_iterations, lambda, btol, Atol, Delta, with_uf,
                                         stop_at, throw_at, rec, rec_cap, out, args...);
}

template <typename... Args>
DeviceVector device_run(const Context &ctx, mi_op *opA, mi_op *opAt, const DeviceVector &b, size_t max_iterations,
                        double lambda, double btol, double Atol, double Delta, bool with_uf, size_t stop_at,
                        size_t throw_at, double *rec, size_t rec_cap, LsqrObsOut *out, Args &...args) {
  LA::LinearOperator<DeviceVector, DeviceVector, Args...> A = MI355::DeviceOperator{opA};
  LA::LinearOperator<DeviceVector, DeviceVector, Args...> At = MI355::DeviceOperator{opAt};
  LA::InnerProduct<DeviceVector, double, Args...> ip = MI355::FrobeniusInnerProduct{};
  mi_fusion_counters f0, f1;
  size_t c0 = 0, c1 = 0;
  ctx.synchronize();
  MI355::check(mi_ctx_fusion_counters(ctx.get(), &f0));
  MI355::check(mi_ctx_sync_count(ctx.get(), &c0));
  const auto t0 = std::chrono::steady_clock::now();
  DeviceVector x = observed_lsqr<DeviceVector, Args...>(A, At, b, ip, max_iterations, lambda, btol, Atol, Delta, with_uf,
                                                        stop_at, throw_at, rec, rec_cap, out, args...);
  MI355::check(mi_ctx_sync_count(ctx.get(), &c1));
  ctx.synchronize();
  out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  MI355::check(mi_ctx_fusion_counters(ctx.get(), &f1));
  out->fused_lsqr_solves = f1.fused_lsqr_solves - f0.fused_lsqr_solves;
  out->generic_lsqr_solves = f1.generic_lsqr_solves - f0.generic_lsqr_solves;
  out->syncs = c1 - c0;
  return x;
}

}  // namespace

// device = 0: HostVec, plain callables (the reference's arithmetic); device = 1: DeviceVector, tagged callables on two CSR
// operators (A and A' of the tridiagonal); no_fused != 0 sets the context switch NO_FUSED_LSQR_OBSERVER.
// pack != 0: Args = {size_t, Vec}.  user_function == 0: the call without a user function (the un-observed solve).
// repeats > 1 (device): the solve is repeated on the one context and the last run reported (benchmarks).
// throw_at != ~0 (device): the user function throws in that pass; the entry point reports -3 if (and only if) the
// exception reached it, then runs the SAME solve again on the same context without the throw and returns that one's
// results.
extern "C" int hl_observed_tridiag(int device, int pack, size_t n, const double *lo, const double *di, const double *up,
                                   const double *b, size_t max_iterations, double lambda, double btol, double Atol,
                                   double Delta, int user_function, size_t stop_at, size_t throw_at, int no_fused,
                                   int repeats, double *rec, size_t rec_cap, double *x_out, LsqrObsOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    size_t counter = 0;
    const bool uf = user_function != 0;
    if (!device) {
      HostVec cache(3);
      HostVec x = pack ? host_run<size_t, HostVec>(n, lo, di, up, b, max_iterations, lambda, btol, Atol, Delta, uf,
                                                   stop_at, throw_at, rec, rec_cap, out, counter, cache)
                       : host_run<>(n, lo, di, up, b, max_iterations, lambda, btol, Atol, Delta, uf, stop_at, throw_at,
                                    rec, rec_cap, out);
      out->counter = counter;
      std::memcpy(x_out, x.d.data(), n * sizeof(double));
      return 0;
    }
    Context ctx(0);
    if (no_fused) MI355::check(mi_ctx_set_option(ctx.get(), "NO_FUSED_LSQR_OBSERVER", 1));
    // CSR of A and of A'
    std::vector<int32_t> rp(n + 1), cl, rpt(n + 1), clt;
    std::vector<double> vl, vlt;
    for (size_t i = 0; i < n; ++i) {
      rp[i] = (int32_t)cl.size();
      rpt[i] = (int32_t)clt.size();
      if (i > 0) {
        cl.push_back((int32_t)i - 1), vl.push_back(lo[i]);
        clt.push_back((int32_t)i - 1), vlt.push_back(up[i - 1]);
      }
      cl.push_back((int32_t)i), vl.push_back(di[i]);
      clt.push_back((int32_t)i), vlt.push_back(di[i]);
      if (i + 1 < n) {
        cl.push_back((int32_t)i + 1), vl.push_back(up[i]);
        clt.push_back((int32_t)i + 1), vlt.push_back(lo[i + 1]);
      }
    }
    rp[n] = (int32_t)cl.size();
    rpt[n] = (int32_t)clt.size();
    mi_csr *A = nullptr, *At = nullptr;
    MI355::check(mi_csr_create(ctx.get(), n, cl.size(), rp.data(), cl.data(), vl.data(), &A));
    MI355::check(mi_csr_create(ctx.get(), n, clt.size(), rpt.data(), clt.data(), vlt.data(), &At));
    mi_op *opA = nullptr, *opAt = nullptr;
    MI355::check(mi_op_create_csr(ctx.get(), A, 1, &opA));
    MI355::check(mi_op_create_csr(ctx.get(), At, 1, &opAt));
    int rc = 0;
    {
      DeviceVector bv(ctx, b, n), cache(ctx, std::vector<double>(3, 1.0));
      auto run = [&](size_t thr) {
        counter = 0;
        return pack ? device_run<size_t, DeviceVector>(ctx, opA, opAt, bv, max_iterations, lambda, btol, Atol, Delta,
                                                       uf, stop_at, thr, rec, rec_cap, out, counter, cache)
                    : device_run<>(ctx, opA, opAt, bv, max_iterations, lambda, btol, Atol, Delta, uf, stop_at, thr,
                                   rec, rec_cap, out);
      };
      if (throw_at != kNever) {
        try {
          (void)run(throw_at);
        } catch (const std::runtime_error &e) {
          if (std::string(e.what()) == "the user function threw") rc = -3;
          else throw;
        }
      }
      for (int rep = 1; rep < repeats; ++rep) (void)run(kNever);
      DeviceVector x = run(kNever);
      out->counter = counter;
      const std::vector<double> xh = x.to_host();
      std::memcpy(x_out, xh.data(), n * sizeof(double));
    }
    mi_op_destroy(opA);
    mi_op_destroy(opAt);
    mi_csr_destroy(A);
    mi_csr_destroy(At);
    return rc;
  } catch (const std::invalid_argument &e) {
    g_msg = e.what();
    return -1;
  } catch (const std::exception &e) {
    g_msg = e.what();
    return -2;
  }
}
