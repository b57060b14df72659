"""Cost of a user function in the inner solve: microseconds per STPCG iteration on the bench workload (cfg2, the Stiefel(n,3)
Rayleigh-quotient Hessian on a 3-D Laplacian, bench.py's parameters) for

  (a) the un-observed fused solve                                   mi_stpcg through capi
  (b) the observed fused solve, observer only counts                STPCG<DeviceVector> + user function (this build)
  (x) the same template call with NO_FUSED_OBSERVER=1               the generic loop of this build (cross-check of (c))
  (c) the same template call on ANOTHER build (--parent DIR)        the generic loop users had before mi_stpcg_observed

Every leg is a child process of its own (a library build per process), started in turn `--reps` times: the legs are
interleaved, the figure of a leg is the MEDIAN over its repetitions of the median over `--calls` timed solves (after
`--warmup` untimed ones) of wall time / iterations, the device drained before and after each solve.

  python tools/bench_observer.py [--grid 100 100 100] [--steps 20] [--reps 5] [--parent DIR] [--out profiles/observer_ab.md]

--parent DIR: a checkout of the other commit with optimization_amd/libmi355opt.so built in it and
libharness_observer_parent.so (tests/cpp/harness_observer.cpp of THIS tree compiled against ITS headers and library).
`python tools/bench_observer.py --prepare-parent DIR [--parent-rev REV]` makes one (no GPU needed; REV defaults to HEAD^):
  git archive REV | tar -x -C DIR
  (cd DIR && python -c "from optimization_amd import build as b; b.build(); b.build_wlgen()")
  g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared -Wall -Wno-type-limits -I DIR/optimization_amd/include -I DIR/oracle \
      -I DIR/include tests/cpp/harness_observer.cpp -o DIR/libharness_observer_parent.so -L DIR/optimization_amd -lmi355opt \
      -Wl,-rpath,DIR/optimization_amd -Wl,-rpath,/opt/rocm/lib
The harness source only uses what the older template layer has too (there the user function selects the generic loop)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prepare_parent(dirname, rev):
    d = os.path.abspath(dirname)
    os.makedirs(d, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", d], input=tar, check=True)
    subprocess.run([sys.executable, "-c", "from optimization_amd import build as b; b.build(); b.build_wlgen()"], cwd=d, check=True)
    lib = os.path.join(d, "optimization_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-type-limits",
                    "-I", os.path.join(lib, "include"), "-I", os.path.join(d, "oracle"), "-I", os.path.join(d, "include"),
                    os.path.join(ROOT, "tests", "cpp", "harness_observer.cpp"), "-o",
                    os.path.join(d, "libharness_observer_parent.so"), "-L", lib, "-lmi355opt", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    print("prepared", d, "at", rev)


def child(a):
    root = os.path.abspath(a.pkgroot) if a.pkgroot else ROOT
    sys.path.insert(0, root)  # (leg c: the other build's own package and library)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from optimization_amd import capi, workloads as wl
    import observer_py
    # the build under the clock must be the one asked for (a PYTHONPATH, an installed copy or MI355OPT_LIB would time another)
    assert os.path.abspath(capi.LIB_PATH).startswith(root + os.sep), (capi.LIB_PATH, root)
    if a.harness:
        observer_py.LIB = a.harness
    nx, ny, nz = a.grid
    n, p = nx * ny * nz, 3
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    Xb, _ = wl.stiefel_bench_iterate(nx, ny, nz, p, eps=1e-3, seed=7)
    c = capi.Context(0)
    if a.leg == "x":
        c.set_option("NO_FUSED_OBSERVER", 1)
    A = c.csr(n, rowptr, col, val)
    prob = c.stiefel_rq(A, n, p)
    g, H = prob.model(c.upload(Xb))
    kw = dict(Delta=1e3, kappa_fgr=1e-12, theta=1.0)
    us, info = [], {}
    if a.leg == "a":
        for i in range(a.warmup + a.calls):
            c.sync()
            t0 = time.perf_counter()
            r = c.stpcg(g, H, max_iterations=a.steps, **kw)
            c.sync()
            dt = time.perf_counter() - t0
            assert r["iterations"] == a.steps
            if i >= a.warmup:
                us.append(1e6 * dt / a.steps)
    else:
        h = observer_py.ObserverHarness()
        h.on(c, g, H, kw["Delta"], a.steps, kw["kappa_fgr"], kw["theta"], reps=a.warmup, want_s=False)
        r = h.on(c, g, H, kw["Delta"], a.steps, kw["kappa_fgr"], kw["theta"], reps=a.calls, want_s=False)
        assert r["rc"] == 0 and r["iterations"] == a.steps and r["calls"] == a.steps, (r["rc"], h.err())
        us = [1e6 * s / a.steps for s in r["seconds"]]
        info = dict(fused=r["fused_stpcg_solves"], generic=r["generic_stpcg_solves"], syncs=r["syncs"])
        assert (info["fused"], info["generic"]) == ((1, 0) if a.leg == "b" else (0, 1)), info
    print(json.dumps(dict(leg=a.leg, us=statistics.median(us), min=min(us), max=max(us), device=c.device_name(), **info)))
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=3, default=[100, 100, 100])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--harness", default=None)
    ap.add_argument("--pkgroot", default=None)
    ap.add_argument("--prepare-parent", default=None)
    ap.add_argument("--parent-rev", default="HEAD^")
    a = ap.parse_args()
    if a.prepare_parent:
        return prepare_parent(a.prepare_parent, a.parent_rev)
    if a.leg:
        return child(a)
    legs = ["a", "b", "x"] + (["c"] if a.parent else [])
    res = {leg: [] for leg in legs}
    dev = ""
    for rep in range(a.reps):
        for leg in legs:
            env = dict(os.environ)
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--calls", str(a.calls), "--grid"] + [str(x) for x in a.grid]
            if leg == "c":
                cmd += ["--pkgroot", os.path.abspath(a.parent), "--harness", os.path.join(os.path.abspath(a.parent), "libharness_observer_parent.so")]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"leg {leg} failed (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            d = json.loads(r.stdout.strip().splitlines()[-1])
            res[leg].append(d)
            dev = d["device"]
            print(f"rep {rep} leg {leg}: {d['us']:.1f} us/iteration (min {d['min']:.1f}, max {d['max']:.1f})", flush=True)
    med = {leg: statistics.median(d["us"] for d in res[leg]) for leg in legs}
    names = dict(a="(a) un-observed fused solve (mi_stpcg)", b="(b) observed fused solve (mi_stpcg_observed, counting observer)",
                 x="(x) this build with NO_FUSED_OBSERVER=1: generic loop (cross-check of (c))",
                 c="(c) the same template call on the parent build: generic loop")
    lines = ["# User function in the inner solve: cost per STPCG iteration", "",
             f"Box: {dev}.  Workload: Stiefel({a.grid[0] * a.grid[1] * a.grid[2]},3) Rayleigh-quotient Hessian on the "
             f"{a.grid[0]}x{a.grid[1]}x{a.grid[2]} Laplacian, Delta 1e3, kappa_fgr 1e-12, theta 1, {a.steps} iterations per solve.",
             f"Command: `python tools/bench_observer.py --steps {a.steps} --reps {a.reps} --calls {a.calls} --warmup {a.warmup}"
             + (" --parent <checkout of the parent commit>`" if a.parent else "`"),
             f"Legs interleaved, one process each; median over {a.reps} repetitions of the median over {a.calls} solves "
             f"({a.warmup} warm-up solves), wall time with the device drained before and after.", "",
             "| leg | us per iteration | repetitions |", "|---|---|---|"]
    for leg in legs:
        lines.append(f"| {names[leg]} | {med[leg]:.1f} | {' '.join('%.1f' % d['us'] for d in res[leg])} |")
    lines += ["", f"(b) / (a) = {med['b'] / med['a']:.2f} (the hope was <= 1.3: one small kernel and one polled wait per pass)."]
    if "c" in med:
        lines.append(f"(b) / (c) = {med['b'] / med['c']:.2f}: the observed fused solve against what a user function cost before "
                     f"({'faster' if med['b'] < med['c'] else 'NOT faster'}).")
    lines.append(f"Host synchronisations per solve: (b) {res['b'][-1].get('syncs')}, (x) {res['x'][-1].get('syncs')}.")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
