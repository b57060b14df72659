// stpcg_kernels.inc -- the two kernels of a fused STPCG iteration (stpcg.hip), included as k_cg_update /
// k_cg_pupdate, as k_cg_update_s80 / k_cg_pupdate_s80 with the scalar-register budget capped at 80 (stpcg.hip says
// why), and as k_cg_update_ns / k_cg_update_ns_s80, the A-step of an odd iteration of the deferred-s form.  Textual inclusion, not a shared __device__ body: the first pair -- the single-GPU step -- must keep the exact
// code it was tuned with.

template <int PRE, bool FROM_SLOTS, int KC = 3, class FOLD = NoFold>
__global__ __launch_bounds__(kBlock) CG_KERNEL_ATTR void CG_UPDATE_NAME(size_t n, CgConst cc, const CgState *__restrict__ st_in,
                                                      CgState *__restrict__ st_out,
                                                      const double *__restrict__ partials_a, int nparts_a,
                                                      const double *__restrict__ slots,
                                                      const double *__restrict__ p,
                                                      const double *__restrict__ Hp,
                                                      const double *__restrict__ pre,
                                                      double *__restrict__ s, double *__restrict__ r,
                                                      double *__restrict__ v,
                                                      double *__restrict__ partials_b, DirGramArgs dg,
                                                      FOLD fold) {
  __shared__ double lds[3 * (kWaves + 1)];
  static_assert(KC >= 3 && KC <= 3 * (kWaves + 1), "3 curvature dots + at most 36 Gram components (p <= 8)");
  CgState cs = load_state(st_in);
  if (cs.mode == CG_DONE) {
    if (blockIdx.x == 0 && threadIdx.x == 0) store_state(st_out, cs);
    return;
  }
  FOLD_STAMP(0);
  const size_t n2 = n >> 1, stride = (size_t)gridDim.x * kBlock;
  const size_t i0 = (size_t)blockIdx.x * kBlock + threadIdx.x;
  // (plain grid-stride walk: the balanced ragged step of k_cg_pupdate costs this kernel 0.5 us)
  auto next_of = [&](size_t i_) -> size_t { return i_ + stride; };
  const size_t ifirst = i0;
  // software prefetch of the first grid-stride step: its HBM latency overlaps the prologue's
  // reduction (tools/microbench/prologue.hip: hides the ~2.2 us prologue completely)
  // (issued BEHIND the prologue's row loads: loads return in order, so the reduction is not held up by them)
  double2 hv0 = make_double2(0, 0), rv0 = hv0;
  // (folded exchange: wave 0 pushes and polls the mailbox, and a wave's memory operations complete in order -- its
  // prefetch waits until the exchange is through, so that the push's release and the poll are not queued behind it)
  // (sharded step at one rank 61.0 -> 60.5 us)
  constexpr bool kFolded = !std::is_same<FOLD, NoFold>::value;
  auto prefetch_now = [&] {
    if (PRE != PRE_BLOCK3 && ifirst < n2) {
      hv0 = reinterpret_cast<const double2 *>(Hp)[ifirst];
      rv0 = reinterpret_cast<double2 *>(r)[ifirst];
    }
  };
  auto prefetch = [&] {
    if (kFolded && threadIdx.x < 64) return;
    prefetch_now();
  };
  double d[KC];
  if (FROM_SLOTS) {
    prefetch_now();
#pragma unroll
    for (int i = 0; i < KC; ++i) d[i] = slots[i];
  } else {
    reduce_rows<KC>(partials_a, nparts_a, d, lds, prefetch);
    // several ranks, peer-memory layer: the sum over the ranks completes HERE instead of in an exchange kernel of its
    // own in front of this one (comm_ipc.h; every rank runs this kernel with the same replicated state)
    fold_maybe<KC>(d, fold, lds);
    if (kFolded && threadIdx.x < 64) prefetch_now();
    if (!kFolded) FOLD_STAMP(1);  // (experiment builds: the prologue's re-reduction is through)
  }
  step_a(cs, cc, d[0], d[1], d[2]);
  if (!kFolded) FOLD_STAMP(5);    // (scalar recurrences done: the streaming part begins)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    store_state(st_out, cs);
    if (KC > 3 && cs.mode == CG_RUN) {  // G(r) += alpha G(Hp)  (r += alpha Hp, :377)
#pragma unroll
      for (int i = 0; i < KC - 3; ++i)
        if (i < dg.ns) dg.gdir[i] = dg.gdir[i] + cs.alpha * d[3 + i];
    }
  }

  const int mode = cs.mode;
  double acc[1] = {0};
  if (mode == CG_APPLY_SIGMA) {
    // (CG_UPDATE_SIGMA 0 -- deferred-s form, odd iteration: s still lacks alpha_k-1 p_k-1, which has to go in FIRST; the
    // direction kernel behind this one has the other direction buffer and applies both, stpcg.hip k_cg_pupdate_ds.  Decided
    // where the file is included: a flag among the arguments, or a test of s, costs the instantiations that sit at 80
    // SGPRs two more)
    if (!CG_UPDATE_SIGMA) return;
    const double sigma = cs.sigma;
    for (size_t i = i0; i < n2; i += stride) {
      const double2 pv = reinterpret_cast<const double2 *>(p)[i];
      double2 sv = reinterpret_cast<double2 *>(s)[i];
      sv.x += sigma * pv.x; sv.y += sigma * pv.y;
      reinterpret_cast<double2 *>(s)[i] = sv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) s[n - 1] += sigma * p[n - 1];
    return;
  }
  if (mode == CG_KERNEL_PENDING) {
    for (size_t i = i0; i < n2; i += stride) {
      const double2 pv = reinterpret_cast<const double2 *>(p)[i];
      const double2 rv = reinterpret_cast<const double2 *>(r)[i];
      acc[0] += pv.x * rv.x; acc[0] += pv.y * rv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) acc[0] += p[n - 1] * r[n - 1];
  } else {  // CG_RUN
    const double alpha = cs.alpha;
    if (PRE == PRE_BLOCK3) {
      const size_t nb = n / 3;
      for (size_t b = i0; b < nb; b += stride) {
        double rr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const size_t i = 3 * b + c;
          rr[c] = r[i] + alpha * Hp[i];
          r[i] = rr[c];
        }
        const double *M = pre + 9 * b;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double vv = M[3 * c] * rr[0] + M[3 * c + 1] * rr[1] + M[3 * c + 2] * rr[2];
          v[3 * b + c] = vv;
          acc[0] += rr[c] * vv;
        }
      }
    } else {
      double2 hv = hv0, rv = rv0;
      for (size_t i = ifirst; i < n2;) {
        const size_t inext = next_of(i);
        double2 hn = hv, rn = rv;
        if (inext < n2) {  // next step's operands are in flight while this one is computed
          hn = reinterpret_cast<const double2 *>(Hp)[inext];
          rn = reinterpret_cast<double2 *>(r)[inext];
        }
        rv.x += alpha * hv.x; rv.y += alpha * hv.y;
        reinterpret_cast<double2 *>(r)[i] = rv;
        if (PRE != PRE_EXTERNAL) {
          double2 vv = rv;
          if (PRE == PRE_DIAG) {
            const double2 dd = reinterpret_cast<const double2 *>(pre)[i];
            vv.x = dd.x * rv.x; vv.y = dd.y * rv.y;
            reinterpret_cast<double2 *>(v)[i] = vv;
          }
          acc[0] += rv.x * vv.x; acc[0] += rv.y * vv.y;
        }
        i = inext; hv = hn; rv = rn;
      }
      if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const size_t i = n - 1;
        const double rv = r[i] + alpha * Hp[i];
        r[i] = rv;
        if (PRE != PRE_EXTERNAL) {
          double vv = rv;
          if (PRE == PRE_DIAG) { vv = pre[i] * rv; v[i] = vv; }
          acc[0] += rv * vv;
        }
      }
    }
    if (PRE == PRE_EXTERNAL) return;  // v = P(r) and <r,v> follow (k_cg_dot_rv)
  }
  block_partials_store<1>(acc, lds, partials_b);
  FOLD_STAMP(6);
}

template <bool FROM_SLOTS, int SP, class FOLD = NoFold>
__global__ __launch_bounds__(kBlock) CG_KERNEL_ATTR void CG_PUPDATE_NAME(size_t n, CgConst cc, const CgState *__restrict__ st_in,
                                                       CgState *__restrict__ st_out,
                                                       const double *__restrict__ partials_b, int nparts_b,
                                                       const double *__restrict__ slots,
                                                       const double *__restrict__ v,
                                                       double *__restrict__ p, double *__restrict__ s,
                                                       HostStatus *hs, double *__restrict__ trace,
                                                       size_t trace_cap, DirGramArgs dg, FOLD fold) {
  __shared__ double lds[DirGramLds<SP>::value];
  CgState cs = load_state(st_in);
  const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
  if (cs.mode == CG_DONE) {
    if (leader) store_state(st_out, cs);
    return;
  }
  const int mode_in = cs.mode;
  const size_t n2 = n >> 1, stride = (size_t)gridDim.x * kBlock;
  const size_t i0 = (size_t)blockIdx.x * kBlock + threadIdx.x;
  // The walk over the n2 double2 elements: whole grid-stride steps up to cc.rag0, then the RAGGED rest -- plain
  // grid-stride gives the first workgroups one element per thread more than the last ones (cfg2: 2.86 steps, 441
  // workgroups walk 3, 71 walk 2) and the kernel ends with the busy ones alone.  Here every workgroup takes the same
  // share of it, one contiguous piece of cc.rag_per elements (20.9 -> 20.3 us; dealing it out in 64-element chunks
  // round-robin was slower than the plain walk, and the same thing in k_cg_update costs that kernel 0.5 us).
  const size_t tail0 = cc.rag0, per = cc.rag_per;
  const size_t irem = (threadIdx.x < per) ? tail0 + (size_t)blockIdx.x * per + threadIdx.x : n2;
  auto next_of = [&](size_t i_) -> size_t {
    const size_t j_ = i_ + stride;
    return j_ < tail0 ? j_ : ((i_ < tail0 && irem < n2) ? irem : n2);
  };
  const size_t ifirst = i0 < tail0 ? i0 : (irem < n2 ? irem : n2);
  // prefetch of the first grid-stride step: overlaps the prologue's reduction, and is issued BEHIND the
  // prologue's row loads (loads return in order, so the reduction is not held up by it)
  double2 vv0 = make_double2(0, 0), pv0 = vv0, sv0 = vv0;
  constexpr int SPN = SP > 0 ? SP : 1;
  double rv0[SPN], rp0[SPN], rs0[SPN], rx0[SPN], ry0[SPN];  // SP > 0: the same prefetch, one row per lane
#pragma unroll
  for (int c = 0; c < SPN; ++c) { rv0[c] = 0; rp0[c] = 0; rs0[c] = 0; rx0[c] = 0; ry0[c] = 0; }
  // (deferring wave 0's prefetch behind the exchange as k_cg_update does costs 0.3 us here: one value, short poll)
  auto prefetch_now = [&] {
    if (SP > 0) {
      if (mode_in == CG_RUN && i0 < n / SPN) {
#pragma unroll
        for (int c = 0; c < SPN; ++c) {
          rv0[c] = v[i0 * SPN + c];
          rp0[c] = p[i0 * SPN + c];
          rs0[c] = s[i0 * SPN + c];
          rx0[c] = dg.X[i0 * SPN + c];
          ry0[c] = dg.Y[i0 * SPN + c];
        }
      }
    } else if (ifirst < n2) {
      const size_t q0 = halo_phys(fold, ifirst);  // (== ifirst unless this launch pushes halo rows early: comm_ipc.h)
      vv0 = reinterpret_cast<const double2 *>(v)[q0];
      pv0 = reinterpret_cast<double2 *>(p)[q0];
      sv0 = reinterpret_cast<double2 *>(s)[q0];
    }
  };
  double red[1] = {0};
  if (mode_in != CG_APPLY_SIGMA && !FROM_SLOTS) {
    reduce_rows<1>(partials_b, nparts_b, red, lds, prefetch_now);
    fold_maybe<1>(red, fold, lds);  // (as in k_cg_update)
  } else {
    prefetch_now();
    if (mode_in != CG_APPLY_SIGMA) red[0] = slots[0];
  }
  step_b(cs, cc, red[0]);
  cs.launches = cs.launches + 1;
  if (leader) {
    store_state(st_out, cs);
    if (mode_in == CG_RUN && trace && cs.k - 1 < trace_cap) {
      const size_t k = (size_t)(cs.k - 1);
      trace[k] = cs.alpha;
      trace[trace_cap + k] = cs.beta;
      trace[2 * trace_cap + k] = cs.kappa;
      trace[3 * trace_cap + k] = cs.rv;
    }
    publish(hs, cs.launches, cs.mode == CG_DONE);
    if (SP == 0 && dg.gdir && mode_in == CG_RUN && cs.mode == CG_RUN) {  // G(p) = -G(r) + beta G(p)  (:420)
      for (int i = 0; i < dg.ns; ++i) dg.gdir[SLOT_GDIR_P + i] = -dg.gdir[i] + cs.beta * dg.gdir[SLOT_GDIR_P + i];
    }
  }
  if (mode_in == CG_KERNEL_PENDING) {
    const double sigma = cs.sigma;
    for (size_t i = i0; i < n2; i += stride) {
      const double2 pv = reinterpret_cast<const double2 *>(p)[i];
      double2 sv = reinterpret_cast<double2 *>(s)[i];
      sv.x += sigma * pv.x; sv.y += sigma * pv.y;
      reinterpret_cast<double2 *>(s)[i] = sv;
    }
    if ((n & 1) && leader) s[n - 1] += sigma * p[n - 1];
  } else if (mode_in == CG_RUN) {
    // s = s + alpha p (:374) is applied HERE, next to the direction update, not in k_cg_update: both need
    // p, so p is read once per iteration instead of twice (8 N bytes saved; same arithmetic, same bits).
    // It is applied whatever the B-step decided; p = -v + beta p (:420) only if the solve goes on.
    const double alpha = cs.alpha, beta = cs.beta;
    const bool dir = cs.mode == CG_RUN;
    if (SP > 0) {
      const size_t nrows = n / SPN;
      double Sm[SPN * SPN], G[SPN * SPN];
#pragma unroll
      for (int i = 0; i < SPN * SPN; ++i) { Sm[i] = dg.S[i]; G[i] = 0; }
      double rv[SPN], rp[SPN], rs[SPN], x[SPN], y[SPN];
#pragma unroll
      for (int c = 0; c < SPN; ++c) { rv[c] = rv0[c]; rp[c] = rp0[c]; rs[c] = rs0[c]; x[c] = rx0[c]; y[c] = ry0[c]; }
      for (size_t row = i0; row < nrows;) {
        const size_t rnext = row + stride;
        double vn[SPN], pn[SPN], sn[SPN], xn[SPN], yn[SPN];
#pragma unroll
        for (int c = 0; c < SPN; ++c) { vn[c] = rv[c]; pn[c] = rp[c]; sn[c] = rs[c]; xn[c] = x[c]; yn[c] = y[c]; }
        if (rnext < nrows) {
#pragma unroll
          for (int c = 0; c < SPN; ++c) {
            vn[c] = v[rnext * SPN + c];
            pn[c] = p[rnext * SPN + c];
            sn[c] = s[rnext * SPN + c];
            xn[c] = dg.X[rnext * SPN + c];
            yn[c] = dg.Y[rnext * SPN + c];
          }
        }
#pragma unroll
        for (int c = 0; c < SPN; ++c) {
          rs[c] = rs[c] + alpha * rp[c];
          s[row * SPN + c] = rs[c];
        }
        if (dir) {
#pragma unroll
          for (int c = 0; c < SPN; ++c) {
            rp[c] = -rv[c] + beta * rp[c];
            p[row * SPN + c] = rp[c];
          }
#pragma unroll
          for (int b = 0; b < SPN; ++b) {
            double t = 0;
#pragma unroll
            for (int a = 0; a < SPN; ++a) t += rp[a] * Sm[a * SPN + b];  // (p S)_b, as the Hessian pass forms it
#pragma unroll
            for (int a = 0; a < SPN; ++a) G[a * SPN + b] += y[a] * rp[b] - x[a] * t;
          }
        }
        row = rnext;
#pragma unroll
        for (int c = 0; c < SPN; ++c) { rv[c] = vn[c]; rp[c] = pn[c]; rs[c] = sn[c]; x[c] = xn[c]; y[c] = yn[c]; }
      }
      if (dir) store_sym_partials<SPN>(G, lds, dg.gpartials);
      return;
    }
    double2 vv = vv0, pv = pv0, sv = sv0;
    bool pushed = false;  // (FoldPush: this thread stored rows of the new direction into a neighbour's halo)
    // L: the logical element of the grid-stride walk, q: where it lives (q == L except in the early form of the halo
    // push, which starts the walk at the rows the neighbours need)
    for (size_t L = ifirst; L < n2;) {
      const size_t Lnext = next_of(L), q = halo_phys(fold, L);
      double2 vn = vv, pn = pv, sn = sv;
      if (Lnext < n2) {
        const size_t qn = halo_phys(fold, Lnext);
        vn = reinterpret_cast<const double2 *>(v)[qn];
        pn = reinterpret_cast<double2 *>(p)[qn];
        sn = reinterpret_cast<double2 *>(s)[qn];
      }
      sv.x = sv.x + alpha * pv.x; sv.y = sv.y + alpha * pv.y;
      reinterpret_cast<double2 *>(s)[q] = sv;
      if (dir) {
        pv.x = -vv.x + beta * pv.x; pv.y = -vv.y + beta * pv.y;
        reinterpret_cast<double2 *>(p)[q] = pv;
        pushed |= halo_push_store(fold, q, pv);
        if (L == ifirst) halo_push_first_step_done(fold);
      }
      L = Lnext; vv = vn; pv = pn; sv = sn;
    }
    if ((n & 1) && leader) {
      s[n - 1] = s[n - 1] + alpha * p[n - 1];
      if (dir) p[n - 1] = -v[n - 1] + beta * p[n - 1];
    }
    // the halo exchange of the next Hessian pass, folded in (comm_ipc.h); `dir` is the same in every workgroup of
    // every rank, so either all of them push or none does -- and the pass that would wait is skipped with them
    if (dir) halo_push_finish(fold, pushed);
  }
}
