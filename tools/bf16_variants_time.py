"""Evaluation forward of the layer variants `gate` and `bilinear` at the AliCCP shape (F = 19, D = 32, H = 4, L = 3, full-size
tables as bench.py's make_config builds them): time per 32,768 resident samples of
  (a) the PARENT commit's library under set_forward_precision("bf16") - there the fp32 layer kernels run (the silent fallback),
  (b) this tree's library under fp32,
  (c) this tree's library under bf16 (csrc/layer_fwd_bf16.hip, MOD 1 / 2: one launch for the stack and the head).
The Python side is the same for all three (the engine asks the library's _supported calls), so (a) needs only the parent's
libsatrans_hip.so: build the parent commit's csrc/ and pass the result as --parent-lib.

One process per library (a library is loaded once per process), started one after the other on an otherwise idle device; the
parent's process runs before AND after this tree's, so drift of the box shows.  In a process: the models are built once, every
(variant, precision) pair is warmed up, then REPS repetitions alternate over the pairs; a repetition is INNER forwards between two
device events.  Reported: the median over the repetitions and their min-max range (the run-to-run spread).
Criterion: median (c) < median (a) by more than the min-max range of (a).

Usage: python tools/bf16_variants_time.py --parent-lib PATH [--parent-commit HASH] [--errors FILE] [--out profiles/bf16_variants_time.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SAMPLES = 32768
VARIANTS = ("sota-gate", "sota-bilinear")


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def child(precisions, reps, inner):
    """Runs in a process of its own (SATRANS_LIB_PATH chooses the library): one JSON line with the times."""
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from satrans_amd import native
    cfg = bench.make_config("aliccp")
    X, _ = bench.synth_batches(N_SAMPLES, 9, cfg=cfg)
    Xd = torch.from_numpy(X).cuda()
    models = {}
    for flag in VARIANTS:
        m = bench.build_model("cpu", cfg["lr"], flag, cfg=cfg)
        m.to("cuda:0")
        m.device = "cuda:0"
        m.eval()
        models[flag] = m
    pairs = [(f, p) for f in VARIANTS for p in precisions]

    def forwards(flag, prec, n):
        m = models[flag]
        m.set_forward_precision(prec)
        eng = m._require_engine()
        for _ in range(n):
            eng.forward(Xd, training=False)

    times = {f"{f}:{p}": [] for f, p in pairs}
    stacked = {}
    for f, p in pairs:
        forwards(f, p, 10)                                # warm-up: code objects, workspaces, scenario tables
        stacked[f"{f}:{p}"] = bool(models[f]._engine._ws[N_SAMPLES].get("acts_stacked"))
    torch.cuda.synchronize()
    for _ in range(reps):
        for f, p in pairs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            forwards(f, p, inner)
            b.record()
            b.synchronize()
            times[f"{f}:{p}"].append(a.elapsed_time(b) / inner)
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "lib": native.LIB_PATH, "sources": native.source_hash(),
                                  "times_ms": times, "bf16_stack_launch": stacked}))


def run_child(lib, precisions, reps, inner, timeout):
    env = dict(os.environ)
    if lib:
        env["SATRANS_LIB_PATH"] = os.path.abspath(lib)
    else:
        env.pop("SATRANS_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", ",".join(precisions), "--reps", str(reps), "--inner", str(inner)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit(f"measurement process failed with status {out.returncode}: nothing more is started")
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def fmt(ts):
    return f"median {median(ts):.4f} ms, min {min(ts):.4f}, max {max(ts):.4f} (range {max(ts) - min(ts):.4f}, {len(ts)} repetitions)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libsatrans_hip.so built from the parent commit's csrc/")
    ap.add_argument("--parent-commit", default="(not given)")
    ap.add_argument("--errors", help="text file with the [bf16-variants] lines tests/test_bf16_variants_gpu.py prints; appended")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_variants_time.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child.split(","), a.reps, a.inner)
        return
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's libsatrans_hip.so is needed for measurement (a)")
    before = run_child(a.parent_lib, ["bf16"], a.reps, a.inner, a.child_timeout)
    this = run_child(None, ["fp32", "bf16"], a.reps, a.inner, a.child_timeout)
    after = run_child(a.parent_lib, ["bf16"], a.reps, a.inner, a.child_timeout)
    lines = [f"tools/bf16_variants_time.py on {this['device']}: evaluation forward (engine.forward, ids resident, head included) per "
             f"{N_SAMPLES:,} samples, AliCCP shape (F = 19, D = 32, H = 4, L = 3, full-size tables)",
             f"parent commit {a.parent_commit} (its library was built from that commit and passed in with --parent-lib); "
             f"this tree: kernel sources sha256 {this['sources'][:16]}",
             f"{a.reps} repetitions of {a.inner} forwards each, alternating over the (variant, precision) pairs of a process; "
             f"processes in order: parent, this tree, parent", ""]
    ok = True
    for flag in VARIANTS:
        ta = before["times_ms"][f"{flag}:bf16"] + after["times_ms"][f"{flag}:bf16"]
        tb, tc = this["times_ms"][f"{flag}:fp32"], this["times_ms"][f"{flag}:bf16"]
        lines += [f"== {flag}",
                  f"(a) parent, precision bf16 (fp32 kernels ran; stack launch: {before['bf16_stack_launch'][flag + ':bf16']}): {fmt(ta)}",
                  f"      before this tree's process: {fmt(before['times_ms'][flag + ':bf16'])}",
                  f"      after  this tree's process: {fmt(after['times_ms'][flag + ':bf16'])}",
                  f"(b) this tree, precision fp32: {fmt(tb)}",
                  f"(c) this tree, precision bf16 (stack launch: {this['bf16_stack_launch'][flag + ':bf16']}): {fmt(tc)}"]
        gain, spread = median(ta) - median(tc), max(ta) - min(ta)
        faster = gain > spread
        ok &= faster
        lines += [f"(a) / (c) = {median(ta) / median(tc):.2f}; (a) - (c) = {gain:.4f} ms against a spread of (a) of {spread:.4f} ms: "
                  f"criterion {'MET' if faster else 'NOT MET'}", ""]
    if a.errors and os.path.exists(a.errors):
        lines += ["Logit errors against the fp32 CPU oracle (tests/test_bf16_variants_gpu.py, synthetic D = 32 / H = 4 / L = 3 models; "
                  "the MetaNet yardstick is the shipped bf16 forward on the same model with flag sota / sota-pos):"]
        lines += [ln[ln.index("[bf16-variants]"):].strip() for ln in open(a.errors) if "[bf16-variants]" in ln and "print(" not in ln]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not ok:
        print("criterion NOT MET for at least one variant")


if __name__ == "__main__":
    main()
