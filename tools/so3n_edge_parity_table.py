"""Render the figures tests/test_gpu_so3n_edges.py logs (SO3N_EDGE_PARITY_LOG=<file>, one JSON object per line) as
the table of profiles/so3n_edge_parity.md:  python tools/so3n_edge_parity_table.py parity.jsonl > table.md"""
import json
import sys


def main(path):
    rows = [json.loads(line) for line in open(path) if line.strip()]
    pieces = [r for r in rows if not r["quantity"].startswith("stpcg")]
    # three Hessian products per case and form: keep the worst
    worst = {}
    for r in pieces:
        k = (r["case"], r["form"], r["quantity"])
        if k not in worst or r["dev_vs_oracle"] > worst[k]["dev_vs_oracle"]:
            worst[k] = r
    print("| case | form | quantity | device vs oracle | device vs longdouble | oracle vs longdouble (floor) | bar |")
    print("|---|---|---|---|---|---|---|")
    for (case, form, q), r in worst.items():
        ld = f"{r['dev_vs_longdouble']:.2e}" if "dev_vs_longdouble" in r else "-"
        print(f"| {case} | {form} | {q} | {r['dev_vs_oracle']:.2e} | {ld} | {r['floor']:.2e} | {r['bar']:.1e} |")
    st = [r for r in rows if r["quantity"].startswith("stpcg")]
    if st:
        print()
        print("| case | preconditioner | solve | iterations | exit | step vs oracle | re-association floor | bar |")
        print("|---|---|---|---|---|---|---|---|")
        for r in st:
            print(f"| {r['case']} | {r['form']} | {r['quantity'][11:]} | {r['iterations']} | {r['exit_reason']} | "
                  f"{r['dev_vs_oracle']:.2e} | {r['floor']:.2e} | {r['bar']:.1e} |")
    plain = lambda q: 1e-10 if q.startswith("stpcg") else 1e-12 if q in ("hess", "precon") else 1e-13
    widened = [r for r in rows if r["bar"] > plain(r["quantity"])]
    big = max((r["dev_vs_oracle"] / r["bar"] for r in rows), default=0.0)
    print()
    print(f"{len(rows)} comparisons; the largest device deviation is {big:.2f} of its bar; {len(widened)} ran at a "
          f"floor-derived bar" + "".join(f": {r['case']} {r['quantity']} at {r['bar']:.1e}" for r in widened) + ".")


if __name__ == "__main__":
    main(sys.argv[1])
