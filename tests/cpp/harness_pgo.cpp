// harness_pgo.cpp -- MI355::PoseGraph the way a client of the drop-in headers calls it (tests/test_gpu_pgo_tnt.py):
//   mode 0  Riemannian::TNT with the tagged accessors and the block-Jacobi preconditioner
//   mode 1  the same run with the objective and the retraction behind plain lambdas: TNT's statement sequence (retract, f,
//           the step scalars in one batched pass) instead of the fused trial chain; the inner solve stays the fused one
//   mode 2  PoseGraph::refine (x_out) -- to be compared with mode 0 bit for bit
//   mode 3  the pipeline of examples/pose_graph_refinement.cpp: spectral initialisation of the rotations,
//           TranslationRecovery::solve, pack, refine; f0 = the objective at the chordal start
// The fusion counters and the number of host synchronisations around the TNT call are reported.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "Optimization/MI355/Device.h"
#include "Optimization/MI355/PoseGraph.h"
#include "Optimization/MI355/SO3.h"
#include "Optimization/Riemannian/TNT.h"

using namespace Optimization;
using MI355::Context;
using MI355::DeviceVector;

static thread_local std::string g_msg;
extern "C" const char *hg_last_error() { return g_msg.c_str(); }

struct PgoTntOut {  // plain data, mirrored by ctypes in tests/harness_pgo_py.py
  double f0, f, gradient_norm;
  size_t outer, inner_total, syncs;
  unsigned long long fused_stpcg, generic_stpcg, fused_trials, generic_trials, generic_inner_products;
  int status;
};

extern "C" int hg_pgo_tnt(int mode, size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *tt,
                          const double *kappa, const double *tau, const double *x0_host, size_t max_iterations, size_t cap,
                          size_t *inner_out, int *accepted_out, double *x_out, PgoTntOut *out) {
  try {
    std::memset(out, 0, sizeof(*out));
    Context ctx(0);
    MI355::PoseGraph pg(ctx, N, E, ei, ej, Rt, tt, kappa, tau);
    Riemannian::TNTParams<double> params;
    params.max_iterations = max_iterations;
    params.relative_decrease_tolerance = 0;  // (only the gradient tolerance, at its default, ends a run)
    params.stepsize_tolerance = 0;
    params.preconditioned_gradient_tolerance = 0;
    DeviceVector x0;
    if (mode == 3) {
      MI355::RotationAveraging rot(ctx, N, E, ei, ej, Rt, kappa);
      const MI355::SpectralResult s = rot.spectral_initialization();
      MI355::TranslationRecovery rec(ctx, N, E, ei, ej, tt, tau, 0);
      const MI355::TranslationResult tr = rec.solve(s.R);
      x0 = pg.pack(s.R, tr.t);
    } else {
      x0 = DeviceVector(ctx, x0_host, 12 * N);
    }
    out->f0 = pg.objective()(x0);
    size_t syncs0 = 0, syncs1 = 0;
    MI355::check(mi_ctx_fusion_counters_reset(ctx.get()));
    MI355::check(mi_ctx_sync_count(ctx.get(), &syncs0));
    std::vector<size_t> inner;
    std::vector<double> rho;
    DeviceVector x;
    if (mode == 2 || mode == 3) {
      const MI355::PoseGraphResult r = pg.refine(x0, params);
      x = r.x;
      out->f = r.f, out->gradient_norm = r.gradient_norm, out->outer = r.outer_iterations, out->inner_total = r.inner_iterations;
      out->status = (int)r.status;
    } else {
      Objective<DeviceVector, double> f = pg.objective();
      Riemannian::Retraction<DeviceVector, DeviceVector> retract = pg.retraction();
      if (mode == 1) {
        const Objective<DeviceVector, double> f_tagged = f;
        f = [f_tagged](const DeviceVector &y) { return f_tagged(y); };
        const Riemannian::Retraction<DeviceVector, DeviceVector> r_tagged = retract;
        retract = [r_tagged](const DeviceVector &y, const DeviceVector &eta) { return r_tagged(y, eta); };
      }
      std::optional<Riemannian::LinearOperator<DeviceVector, DeviceVector>> precon = pg.preconditioner();
      const auto r = Riemannian::TNT<DeviceVector, DeviceVector, double>(f, pg.quadratic_model(), pg.metric(), retract, x0, precon, params);
      x = r.x;
      out->f = r.f, out->gradient_norm = r.gradfx_norm, out->outer = r.inner_iterations.size(), out->status = (int)r.status;
      inner = r.inner_iterations;
      rho = r.gain_ratios;
      for (size_t k : inner) out->inner_total += k;
    }
    MI355::check(mi_ctx_sync_count(ctx.get(), &syncs1));
    mi_fusion_counters fc;
    MI355::check(mi_ctx_fusion_counters(ctx.get(), &fc));
    out->syncs = syncs1 - syncs0;
    out->fused_stpcg = fc.fused_stpcg_solves, out->generic_stpcg = fc.generic_stpcg_solves;
    out->fused_trials = fc.fused_trial_steps, out->generic_trials = fc.generic_trial_steps;
    out->generic_inner_products = fc.generic_inner_products;
    for (size_t k = 0; k < inner.size() && k < cap; ++k) {
      inner_out[k] = inner[k];
      accepted_out[k] = (rho[k] == rho[k] && rho[k] > params.eta1) ? 1 : 0;
    }
    const std::vector<double> xh = x.to_host();
    std::memcpy(x_out, xh.data(), xh.size() * sizeof(double));
    return 0;
  } catch (const std::exception &e) {
    g_msg = e.what();
    return 1;
  }
}
