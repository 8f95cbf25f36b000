#!/usr/bin/env python3
"""jf_qknorm_rope_kv_append (Qwen3's per-head q/k RMSNorm + RoPE + query re-layout + KV append of one layer) at the head geometry
of Qwen3-4B (32 q + 8 kv, D = 128), 2 176 tokens (64 rows x 34), bf16 and f32.  Three things on the same buffers, alternating
round by round in one process, device events around each batch of calls:

  (a) the fused call                                        ops.qknorm_rope_kv_append
  (b) torch normalisation of the q and k slices, then       Qwen2Model._qk_norm_ + ops.rope_kv_append   (the QKNORM_FUSED=0 path)
  (c) jf_rope_kv_append alone                               ops.rope_kv_append                          (the floor: same bytes
                                                                                                          minus two weight rows)

Prints the median and the min..max of the rounds for each, (a)/(b), (a)/(c) and the run-to-run spread of (c).

    python tools/microbench_qknorm_rope.py [rows T]
"""
import statistics
import sys
import types
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from jacobiforcing_amd import ops  # noqa: E402
from jacobiforcing_amd.modeling.qwen2 import Qwen2Config, Qwen2Model  # noqa: E402

nq, nkv, D, eps = 32, 8, 128, 1e-6
R, T = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (64, 34)
ROUNDS, CALLS = 15, 200
if not torch.cuda.is_available():
    sys.exit("microbench_qknorm_rope: needs a GPU (a CPU run says nothing about the kernel)")
dev = "cuda"
N = R * T
S_max = 2048
cfg = Qwen2Config(num_attention_heads=nq, num_key_value_heads=nkv, head_dim=D, rms_norm_eps=eps, qk_norm=True, attention_bias=False)
norm_ = types.SimpleNamespace(cfg=cfg)                                  # _qk_norm_ reads nothing but the config
inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
fr = torch.outer(torch.arange(S_max, dtype=torch.float32), inv)
cos, sin = fr.cos().to(dev), fr.sin().to(dev)
pos = torch.randint(0, 1024, (N,), dtype=torch.int32, device=dev)
slot = (torch.arange(R, device=dev).repeat_interleave(T) * S_max + 100 + torch.arange(T, device=dev).repeat(R)).to(torch.int64)
print(f"# {R} rows x T {T} = {N} tokens, nq {nq}, nkv {nkv}, D {D}; {ROUNDS} rounds x {CALLS} calls each, device events; us per call")
for dtype in (torch.bfloat16, torch.float32):
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(N, (nq + 2 * nkv) * D, device=dev, generator=g).to(dtype)
    qn = (1 + 0.5 * torch.randn(D, device=dev, generator=g)).to(dtype)
    kn = (1 + 0.5 * torch.randn(D, device=dev, generator=g)).to(dtype)
    kc = torch.zeros(R, nkv, S_max, D, dtype=dtype, device=dev)
    vc = torch.zeros_like(kc)
    work = qkv.clone()                                                  # (b) normalises in place: its own copy of the buffer

    def fused():
        return ops.qknorm_rope_kv_append(qkv, T, nq, nkv, D, qn, kn, eps, pos, cos, sin, kc, vc, slot)

    def unfused():
        Qwen2Model._qk_norm_(norm_, work, qn, kn)
        return ops.rope_kv_append(work, T, nq, nkv, D, pos, cos, sin, kc, vc, slot)

    def floor():
        return ops.rope_kv_append(qkv, T, nq, nkv, D, pos, cos, sin, kc, vc, slot)

    # the two routes compute the same thing at the size that is timed (bf16: the torch route rounds twice more)
    qa = fused().float()
    work.copy_(qkv)
    qb = unfused().float()
    err = float((qa - qb).abs().max())
    assert err <= float(qa.abs().max()) * (2.0 ** -6 if dtype == torch.bfloat16 else 2.0 ** -18), err
    variants = (("a fused", fused), ("b torch norm + rope", unfused), ("c rope alone", floor))
    for _, f in variants:
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, f in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                f()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / CALLS)
    med = {k: statistics.median(v) for k, v in times.items()}
    esz = qkv.element_size()
    moved = N * (nq + 2 * nkv) * D * esz * 2                           # every element read once and written once
    print(f"{str(dtype).split('.')[-1]}: max |fused - torch route| on q_out {err:.3g}; {moved / 1e6:.1f} MB moved per call")
    for name, _ in variants:
        v = times[name]
        print(f"  ({name:22s}) median {med[name]:7.2f}  min {min(v):7.2f}  max {max(v):7.2f}   {moved / med[name] / 1e3:6.0f} GB/s")
    c = times["c rope alone"]
    spread = (max(c) - min(c)) / med["c rope alone"]
    print(f"  (a)/(b) = {med['a fused'] / med['b torch norm + rope']:.3f}   (a)/(c) = {med['a fused'] / med['c rope alone']:.3f}   "
          f"run-to-run spread of (c) = {100 * spread:.1f} % of its median")
