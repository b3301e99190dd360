#!/usr/bin/env python3
"""GPU box: the code-touch stride sweep of profiles/code_touch_election_mi355x.md on the PRODUCT library.

bench.py sets no plan options, so this runs bench.py's own main() -- the same step, HBM-cold, the same per-layer
figures -- with a backend whose plans carry option "code_touchers" = T (include/escoin.h), one fresh process per stride:

    python tools/touch_sweep.py [--strides 0,1,2,4,8,16,65535] [--workload resnet50] [--repeats 1]

0 is the rule (csrc/align_rules.h touch_election).  One line per run: the stride, ms per step, us per launch of the
first layers as bench.py reports them (roofline.per_layer)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(stride, bench_argv):
    """This process as one bench run at `stride`: bench.main() with the option on every plan."""
    import bench
    import __graft_entry__ as ge

    class Backend(bench.HipBackend):
        def make_plan(self, shape):
            plan = bench.HipBackend.make_plan(self, shape)
            plan.set_option("code_touchers", stride)
            return plan

    def factory(local_rank):
        pkg = ge.load_package()
        return Backend(pkg, local_rank, pkg.KERNEL_AUTO)

    sys.argv = [os.path.join(ROOT, "bench.py")] + bench_argv
    bench.main(backend_factory=factory, script=os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strides", default="0,1,2,4,8,16,65535")
    ap.add_argument("--workload", default="resnet50")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    bench_argv = ["--full", "--workload", args.workload, "--no-cpu", "--no-extras"]
    if args.one is not None:
        return one(args.one, bench_argv)
    for rep in range(args.repeats):
        for stride in (int(v) for v in args.strides.split(",")):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(stride), "--workload", args.workload],
                                 stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, cwd=ROOT, timeout=600)
            lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{") and '"metric"' in l]
            if out.returncode != 0 or not lines:
                print("stride %d: bench failed (exit %d)" % (stride, out.returncode), flush=True)
                return 1
            d = json.loads(lines[-1])
            layers = " ".join("%s:%.1f" % (l["layer"].split("_")[0][:10], l["us"]) for l in d["roofline"]["per_layer"][:8])
            print("T=%-6d ms/step %.4f  %s  parity %.1e" % (stride, d["ms_per_step"], layers, d["parity_max_rel_err"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
