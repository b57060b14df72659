// harness_observer.cpp -- STPCG with a user function (reference IterativeSolvers.h:50-59, called at :365-369) through
// ONE templated driver compiled twice: on the plain host vector of oracle/template_driver.inc, where the template
// layer's generic loop is bit-identical to the reference (tests/test_cpu_oracle_templates.py), and on
// MI355::DeviceVector with the tagged device callables, where the solve keeps the fused kernels and the user function
// observes it (mi_stpcg_observed).  Per call the user function records
//     k, alpha, <s,s>, <r,r>, <r,v>, <p,p>, <s,p>
// so that pytest can compare what the two see (tests/test_gpu_stpcg_observer.py).  TEST INFRASTRUCTURE ONLY.
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

#define DRV(name) hob_##name
#include "template_driver.inc"  // HostVec (and its drivers under the hob_ prefix, unused here)

using Optimization::MI355::Context;
using Optimization::MI355::DeviceVector;
namespace MI355 = Optimization::MI355;

static thread_local std::string g_msg;
extern "C" const char *hob_last_error() { return g_msg.c_str(); }

namespace {

constexpr int kRecCols = 7;
constexpr size_t kNever = ~(size_t)0;

struct ObsOut {        // plain data, mirrored by ctypes in the test
  size_t nrec;         // calls of the user function
  size_t iterations;
  double M_norm;
  int P_engaged, At_engaged;  // what the user function saw in its P and At arguments (last call; -1: never called)
  int v_is_r;                 // device only: v and r were the same handle in every call
  unsigned long long fused_stpcg_solves, generic_stpcg_solves, generic_inner_products;  // over the solve (device)
  size_t syncs;                                                                        // mi_ctx_sync_count over the solve
};

// the one driver: STPCG<Vec, Mult> with a user function that records, stops at `stop_at` and throws at `throw_at`
template <typename Vec, typename Mult>
Vec observed_solve(const Vec &g, const LA::SymmetricLinearOperator<Vec> &H, const LA::InnerProduct<Vec> &ip,
                   const std::optional<LA::STPCGPreconditioner<Vec, Mult>> &P,
                   const std::optional<LA::LinearOperator<Mult, Vec>> &At, double Delta, size_t max_iterations,
                   double kappa, double theta, size_t stop_at, size_t throw_at, bool record_dots, double *rec,
                   size_t rec_cap, ObsOut *out) {
  out->nrec = 0;
  out->P_engaged = out->At_engaged = -1;
  std::optional<LA::STPCGUserFunction<Vec, Mult>> uf = LA::STPCGUserFunction<Vec, Mult>(
      [&](size_t k, const Vec &, const LA::SymmetricLinearOperator<Vec> &,
          const std::optional<LA::STPCGPreconditioner<Vec, Mult>> &Pk,
          const std::optional<LA::LinearOperator<Mult, Vec>> &Atk, const Vec &s, const Vec &r, const Vec &v, const Vec &p,
          double alpha) {
        if (k == throw_at) throw std::runtime_error("the user function threw");
        out->P_engaged = Pk ? 1 : 0;
        out->At_engaged = Atk ? 1 : 0;
        if constexpr (std::is_same<Vec, DeviceVector>::value) {
          const bool same = v.handle() == r.handle();
          out->v_is_r = out->nrec == 0 ? (same ? 1 : 0) : (out->v_is_r && same ? 1 : 0);
        }
        if (out->nrec < rec_cap) {
          double *row = rec + out->nrec * kRecCols;
          row[0] = (double)k;
          row[1] = alpha;
          for (int c = 2; c < kRecCols; ++c) row[c] = 0;
          if (record_dots) {
            row[2] = s.dot(s);
            row[3] = r.dot(r);
            row[4] = r.dot(v);
            row[5] = p.dot(p);
            row[6] = s.dot(p);
          }
        }
        out->nrec++;
        return k == stop_at;
      });
  double mn = 0;
  size_t it = 0;
  Vec s = LA::STPCG<Vec, Mult>(g, H, ip, mn, it, Delta, max_iterations, kappa, theta, P, At, uf);
  out->M_norm = mn;
  out->iterations = it;
  return s;
}

// device side of a solve: counters and synchronisations over the STPCG call alone
template <typename F>
DeviceVector counted(const Context &ctx, ObsOut *out, F &&solve) {
  mi_fusion_counters f0, f1;
  size_t c0 = 0, c1 = 0;
  MI355::check(mi_ctx_fusion_counters(ctx.get(), &f0));
  MI355::check(mi_ctx_sync_count(ctx.get(), &c0));
  DeviceVector s = solve();
  MI355::check(mi_ctx_sync_count(ctx.get(), &c1));
  MI355::check(mi_ctx_fusion_counters(ctx.get(), &f1));
  out->fused_stpcg_solves = f1.fused_stpcg_solves - f0.fused_stpcg_solves;
  out->generic_stpcg_solves = f1.generic_stpcg_solves - f0.generic_stpcg_solves;
  out->generic_inner_products = f1.generic_inner_products - f0.generic_inner_products;
  out->syncs = c1 - c0;
  return s;
}

}  // namespace

#define HOB_GUARD_END                        \
  }                                          \
  catch (const std::invalid_argument &e) {   \
    g_msg = e.what();                        \
    return -1;                               \
  }                                          \
  catch (const std::exception &e) {          \
    g_msg = e.what();                        \
    return -2;                               \
  }                                          \
  return 0;

// ------------------------------------------------------------------------------------------------
// diagonal Hessian D, optional diagonal preconditioner Minv (oracle_py.stpcg_stop_problem).
//   device = 0: HostVec, plain callables (the reference's arithmetic);
//   device = 1: DeviceVector, tagged callables; no_fused_observer != 0 sets the context switch NO_FUSED_OBSERVER.
//   throw_at != ~0: the user function throws in that pass; the entry point reports -3 if (and only if) the exception
//   reached it, then runs the SAME solve again on the same context without the throw and returns that one's results.
// ------------------------------------------------------------------------------------------------
extern "C" int hob_observed_diag(int device, size_t n, const double *g, const double *D, const double *Minv, double Delta,
                                 size_t max_iterations, double kappa, double theta, size_t stop_at, size_t throw_at,
                                 int record_dots, int no_fused_observer, double *rec, size_t rec_cap, double *s_out,
                                 ObsOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    if (!device) {
      LA::SymmetricLinearOperator<HostVec> H = [&](const HostVec &v) {
        HostVec o(n);
        for (size_t i = 0; i < n; ++i) o.d[i] = D[i] * v.d[i];
        return o;
      };
      LA::InnerProduct<HostVec> ip = [](const HostVec &a, const HostVec &b) { return a.dot(b); };
      std::optional<LA::STPCGPreconditioner<HostVec, Mult>> P;
      if (Minv)
        P = [&](const HostVec &v) {
          HostVec o(n);
          for (size_t i = 0; i < n; ++i) o.d[i] = Minv[i] * v.d[i];
          return std::make_pair(o, Mult());
        };
      const std::optional<LA::LinearOperator<Mult, HostVec>> At;
      HostVec s = observed_solve<HostVec, Mult>(HostVec(g, n), H, ip, P, At, Delta, max_iterations, kappa, theta, stop_at,
                                                throw_at, record_dots != 0, rec, rec_cap, out);
      std::memcpy(s_out, s.d.data(), n * sizeof(double));
      return 0;
    }
    Context ctx(0);
    if (no_fused_observer) MI355::check(mi_ctx_set_option(ctx.get(), "NO_FUSED_OBSERVER", 1));
    DeviceVector gd(ctx, g, n), Dd(ctx, D, n);
    mi_op *op = nullptr;
    MI355::check(mi_op_create_diag(ctx.get(), Dd.handle(), &op));
    mi_precon *pc = nullptr;
    std::optional<DeviceVector> Mi;
    if (Minv) {
      Mi = DeviceVector(ctx, Minv, n);
      MI355::check(mi_precon_create_diag(ctx.get(), Mi->handle(), &pc));
    }
    LA::SymmetricLinearOperator<DeviceVector> H = MI355::DeviceOperator{op};
    LA::InnerProduct<DeviceVector> ip = MI355::FrobeniusInnerProduct{};
    std::optional<LA::STPCGPreconditioner<DeviceVector, Mult>> P;
    if (pc) P = MI355::DeviceSTPCGPreconditioner<Mult>{pc};
    const std::optional<LA::LinearOperator<Mult, DeviceVector>> At;
    int rc = 0;
    if (throw_at != kNever) {
      try {
        (void)observed_solve<DeviceVector, Mult>(gd, H, ip, P, At, Delta, max_iterations, kappa, theta, stop_at, throw_at,
                                                 record_dots != 0, rec, rec_cap, out);
      } catch (const std::runtime_error &e) {
        if (std::string(e.what()) == "the user function threw") rc = -3;
        else throw;
      }
    }
    DeviceVector s = counted(ctx, out, [&] {
      return observed_solve<DeviceVector, Mult>(gd, H, ip, P, At, Delta, max_iterations, kappa, theta, stop_at, kNever,
                                                record_dots != 0, rec, rec_cap, out);
    });
    const std::vector<double> sh = s.to_host();
    std::memcpy(s_out, sh.data(), n * sizeof(double));
    mi_op_destroy(op);
    if (pc) mi_precon_destroy(pc);
    return rc;
  HOB_GUARD_END
}

// ------------------------------------------------------------------------------------------------
// the projected solve (constraint preconditioner + At, IterativeSolvers.h:229-253,381-405) on the inputs of
// oracle_py.projected_stpcg_problem, Multiplier = Vector.  device = 0: host KKT algebra (oracle/kkt_dense.h);
// device = 1: the tagged constraint preconditioner and A' of one device KKT object.
// ------------------------------------------------------------------------------------------------
extern "C" int hob_observed_projected(int device, size_t n, size_t m, const double *g, const double *Pdiag,
                                      const double *Mdiag, const double *A, double Delta, size_t max_iterations,
                                      double kappa, double theta, int record_dots, double *rec, size_t rec_cap,
                                      double *s_out, ObsOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    if (!device) {
      const KktDense K(n, m, A, Mdiag);
      LA::SymmetricLinearOperator<HostVec> H = [&](const HostVec &v) {
        HostVec o(n);
        for (size_t i = 0; i < n; ++i) o.d[i] = Pdiag[i] * v.d[i];
        return o;
      };
      LA::InnerProduct<HostVec> ip = [](const HostVec &a, const HostVec &b) { return a.dot(b); };
      std::optional<LA::STPCGPreconditioner<HostVec, HostVec>> P =
          LA::STPCGPreconditioner<HostVec, HostVec>([&](const HostVec &r) {
            HostVec x(n), l(m);
            K.solve(r.d.data(), x.d.data(), l.d.data());
            return std::make_pair(x, l);
          });
      std::optional<LA::LinearOperator<HostVec, HostVec>> At = LA::LinearOperator<HostVec, HostVec>([&](const HostVec &l) {
        HostVec o(n);
        K.At(l.d.data(), o.d.data());
        return o;
      });
      HostVec s = observed_solve<HostVec, HostVec>(HostVec(g, n), H, ip, P, At, Delta, max_iterations, kappa, theta, kNever,
                                                   kNever, record_dots != 0, rec, rec_cap, out);
      std::memcpy(s_out, s.d.data(), n * sizeof(double));
      return 0;
    }
    Context ctx(0);
    DeviceVector gd(ctx, g, n), Pd(ctx, Pdiag, n);
    mi_op *op = nullptr;
    MI355::check(mi_op_create_diag(ctx.get(), Pd.handle(), &op));
    LA::SymmetricLinearOperator<DeviceVector> H = MI355::DeviceOperator{op};
    LA::InnerProduct<DeviceVector> ip = MI355::FrobeniusInnerProduct{};
    std::vector<double> mi(n);
    for (size_t i = 0; i < n; ++i) mi[i] = 1.0 / Mdiag[i];
    DeviceVector Ad(ctx, A, n * m), Mi(ctx, mi);
    mi_precon *kkt = nullptr;
    MI355::check(mi_precon_create_constraint(ctx.get(), n, m, Ad.handle(), Mi.handle(), &kkt));
    std::optional<LA::STPCGPreconditioner<DeviceVector, DeviceVector>> P =
        LA::STPCGPreconditioner<DeviceVector, DeviceVector>(MI355::DeviceConstraintPreconditioner{kkt, m});
    std::optional<LA::LinearOperator<DeviceVector, DeviceVector>> At =
        LA::LinearOperator<DeviceVector, DeviceVector>(MI355::DeviceConstraintTranspose{kkt, n});
    DeviceVector s = counted(ctx, out, [&] {
      return observed_solve<DeviceVector, DeviceVector>(gd, H, ip, P, At, Delta, max_iterations, kappa, theta, kNever,
                                                        kNever, record_dots != 0, rec, rec_cap, out);
    });
    const std::vector<double> sh = s.to_host();
    std::memcpy(s_out, sh.data(), n * sizeof(double));
    mi_precon_destroy(kkt);
    mi_op_destroy(op);
  HOB_GUARD_END
}

// ------------------------------------------------------------------------------------------------
// The template call on objects that already live on a context of the C ABI (a Stiefel model made through capi.py):
// STPCG<DeviceVector, nullptr_t> with the tagged operator, no preconditioner and a user function that only counts.
// `reps` calls, the device drained before and after each; seconds[i] = wall time of call i.  (tools/bench_observer.py)
// ------------------------------------------------------------------------------------------------
extern "C" int hob_observed_on(void *ctx_handle, void *g_handle, void *op_handle, double Delta, size_t max_iterations,
                               double kappa, double theta, int reps, double *seconds, double *s_out, ObsOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    mi_ctx *c = static_cast<mi_ctx *>(ctx_handle);
    const Context ctx = Context::adopt(c);
    const DeviceVector gd = DeviceVector::view(c, static_cast<mi_vec *>(g_handle));
    LA::SymmetricLinearOperator<DeviceVector> H = MI355::DeviceOperator{static_cast<mi_op *>(op_handle)};
    LA::InnerProduct<DeviceVector> ip = MI355::FrobeniusInnerProduct{};
    const std::optional<LA::STPCGPreconditioner<DeviceVector, Mult>> P;
    const std::optional<LA::LinearOperator<Mult, DeviceVector>> At;
    for (int i = 0; i < reps; ++i) {
      ctx.synchronize();
      const auto t0 = std::chrono::steady_clock::now();
      DeviceVector s = counted(ctx, out, [&] {
        return observed_solve<DeviceVector, Mult>(gd, H, ip, P, At, Delta, max_iterations, kappa, theta, kNever, kNever,
                                                  false, nullptr, 0, out);
      });
      ctx.synchronize();
      if (seconds) seconds[i] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (s_out && i + 1 == reps) {
        const std::vector<double> sh = s.to_host();
        std::memcpy(s_out, sh.data(), sh.size() * sizeof(double));
      }
    }
  HOB_GUARD_END
}
