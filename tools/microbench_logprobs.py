#!/usr/bin/env python3
"""jf_logprobs_rows at the non-greedy verify's shape — 64 x 31 rows x V = 152 064, bf16 and float32, top_n in {0, 1, 5, 20} —
with jf_rs_probs on the same tensor in the same run as the yardstick: both read the same bytes once (0.6 GB bf16 / 1.2 GB
float32, larger than the caches).  Microseconds per call from device events around the call's dispatches, after a warm-up,
the calls of the five kinds alternating; median, min and max over --iters calls, the effective read bandwidth and the ratio to
jf_rs_probs.

    python tools/microbench_logprobs.py [--rows 1984] [--iters 20] [--temperature 0.8]"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from jacobiforcing_amd import _native as N  # noqa: E402
from jacobiforcing_amd import ops  # noqa: E402

TOPS = (0, 1, 5, 20)


def measure(dtype: torch.dtype, rows: int, V: int, temperature: float, iters: int) -> None:
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(3)
    logits = (torch.randn((rows, V), generator=g, device=dev) * 2.5).to(dtype)
    chosen = torch.randint(0, V, (rows,), generator=g, device=dev)
    lib, dt, stream = N.lib(), ops._dtype_code(logits), ops._stream(dev)
    lp = ops.LogprobRows(dev, rows)
    core = ops._OnPolicyCore(rows, dev, [0])                              # jf_rs_probs' buffers, as the steppers hold them
    core.ws = ops._grown(core.ws, int(lib.jf_rs_workspace_bytes(rows, V)))

    def probs():
        core.packed.zero_()
        return lambda: N.check(lib.jf_rs_probs(ops._ptr(logits), dt, rows, V, V, ops._ptr(chosen), temperature, ops._ptr(core.p_draft),
                                               ops._ptr(core.row_max), ops._ptr(core.row_sumexp), ops._ptr(core.packed), ops._ptr(core.ws),
                                               core.ws.numel() * 4, stream), "jf_rs_probs")

    def logprobs(n):
        ws = torch.zeros((int(lib.jf_logprobs_workspace_bytes(rows, V, n)) // 8 + 2,), dtype=torch.float64, device=dev)
        ids, tl = lp.top_ids[:rows * n], lp.top_lp[:rows * n]
        return lambda: N.check(lib.jf_logprobs_rows(ops._ptr(logits), dt, rows, V, V, temperature, ops._ptr(chosen), n, ops._ptr(lp.logprob),
                                                    ops._ptr(lp.rank), ops._ptr(ids) if n else None, ops._ptr(tl) if n else None, ops._ptr(ws),
                                                    ws.numel() * 8, stream), "jf_logprobs_rows")
    kinds = [("jf_rs_probs", probs())] + [(f"jf_logprobs_rows top_n={n}", logprobs(n)) for n in TOPS]
    times = {k: [] for k, _ in kinds}
    for it in range(iters + 3):                                           # three warm-up rounds; the kinds alternate
        for name, call in kinds:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if it >= 3:
                times[name].append(a.elapsed_time(b) * 1e3)
    nbytes = rows * V * logits.element_size()
    base = statistics.median(times["jf_rs_probs"])
    name_dt = "bf16" if dtype == torch.bfloat16 else "f32"
    print(f"{rows} rows x V={V} {name_dt} T={temperature} ({nbytes / 1e6:.0f} MB read once per call): us per call over {iters} calls", flush=True)
    for name, _ in kinds:
        t = times[name]
        med = statistics.median(t)
        print(f"  {name:<28} median {med:9.1f}  min {min(t):9.1f}  max {max(t):9.1f}   {nbytes / med / 1e6:5.2f} TB/s   {med / base:5.2f} x jf_rs_probs",
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64 * 31)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--temperature", type=float, nargs="+", default=[0.8, 1.0])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_logprobs.py measures on the GPU: none found")
    for dtype in (torch.bfloat16, torch.float32):
        for t in args.temperature:
            measure(dtype, args.rows, args.vocab, float(t), args.iters)
