#!/usr/bin/env python3
"""The sampling part of an autoregressive decode step at 64 rows x V = 152 064 bf16 logits: the per-row torch loop of
ModelRunner._run_autoregressive (copied below as it stood before ops.ARSampler existed) against ARSampler.sample, at T = 0.8
plain and with top_k = 50 / top_p = 0.9.  Microseconds per step on the host clock around work that ends in a synchronise (both
sides read their tokens back), five alternating runs per side, median and spread.

--generate: LLM.generate, autoregressive, T = 0.8, 64 requests on the 7B random-init shape, tokens/s with the torch loop
(default) and with JF_AR_SAMPLER=1, three alternating runs per side.

    python tools/microbench_ar_sampler.py [--generate] [--rows 64] [--iters 20]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from jacobiforcing_amd import LLM, SamplingParams, ops  # noqa: E402


def torch_loop(logits: torch.Tensor, t: float, k: int, tp: float) -> list:
    """The rows' loop body of the parent's _run_autoregressive (temperature > 0), line for line."""
    toks = []
    for i in range(logits.shape[0]):
        p = torch.softmax(logits[i:i + 1].float() / t, dim=-1)
        if k:
            v, idx = torch.topk(p, k, dim=-1)
            p = torch.zeros_like(p).scatter_(-1, idx, v)
            p = p / p.sum(dim=-1, keepdim=True).clamp_min(1e-12)
        if tp:
            sp, si = torch.sort(p, dim=-1, descending=True)
            keep = torch.cumsum(sp, dim=-1) <= tp
            keep[..., 0] = True
            sp = sp * keep
            p = torch.zeros_like(p).scatter_(-1, si, sp / sp.sum(dim=-1, keepdim=True).clamp_min(1e-12))
        toks.append(int(torch.argmax(p / torch.empty_like(p).exponential_(1).clamp_min_(1e-10), dim=-1)[0]))
    return toks


def spread(xs):
    return f"median {statistics.median(xs):9.1f}  min {min(xs):9.1f}  max {max(xs):9.1f}"


def sampling_part(rows: int, iters: int) -> None:
    V, dev = 152064, torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(rows, V, generator=g) * 2.5).to(torch.bfloat16).to(dev)
    smp = ops.ARSampler(dev, rows)
    for k, tp in ((0, 0.0), (50, 0.9)):
        settings = [(0.8, k, tp)] * rows
        us = [np.asarray([smp.uniform(1000 + r, j) for r in range(rows)], dtype=np.float32) for j in range(iters)]

        def run_torch():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                torch_loop(logits, 0.8, k, tp)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e6

        def run_hip():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(iters):
                smp.sample(logits, settings, us[j])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e6
        run_torch(), run_hip()                                            # warm-up of both sides
        a, b = [], []
        for _ in range(5):                                                # alternating
            a.append(run_torch())
            b.append(run_hip())
        print(f"rows={rows} V={V} bf16 T=0.8 top_k={k} top_p={tp}: us per step", flush=True)
        print(f"  torch loop   {spread(a)}", flush=True)
        print(f"  ARSampler    {spread(b)}   ({statistics.median(a) / statistics.median(b):.1f}x)", flush=True)


def generate_part(requests: int, max_tokens: int) -> None:
    from jacobiforcing_amd.engine.model_runner import ModelRunner
    from jacobiforcing_amd.modeling.qwen2 import Qwen2Config, Qwen2Weights
    from jacobiforcing_amd.synthetic import humaneval_shaped_prompts
    cfg = Qwen2Config.qwen2_5_coder_7b()
    d = tempfile.mkdtemp()
    (Path(d) / "config.json").write_text(json.dumps(dict(
        vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
        num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
        num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, max_position_embeddings=cfg.max_position_embeddings,
        rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta, tie_word_embeddings=cfg.tie_word_embeddings,
        eos_token_id=-1, pad_token_id=cfg.pad_token_id, model_type="qwen2")))
    ModelRunner.shared_weights = Qwen2Weights(cfg, torch.device("cuda"), dtype=torch.bfloat16, seed=0)
    try:
        llm = LLM(d, tokenizer_path="none", max_model_len=2048, max_num_batched_tokens=65536, max_num_seqs=requests)
    finally:
        ModelRunner.shared_weights = None
    prompts = [p[:400] for p in humaneval_shaped_prompts(requests, seed=4242, vocab_hi=min(151643, cfg.vocab_size - 2))]
    sp = SamplingParams(temperature=0.8, max_tokens=max_tokens, ignore_eos=True)

    def run(device_path: bool) -> float:
        os.environ["JF_AR_SAMPLER"] = "1" if device_path else "0"
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = llm.generate(prompts, sp, use_tqdm=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return sum(len(r["token_ids"]) for r in res) / dt
    run(False), run(True)                                                 # untimed: loads the GEMM shapes of both paths
    a, b = [], []
    for _ in range(3):
        a.append(run(False))
        b.append(run(True))
    os.environ.pop("JF_AR_SAMPLER", None)
    print(f"LLM.generate autoregressive T=0.8, {requests} requests x {max_tokens} tokens, 7B random-init bf16 (prefill included): tokens/s", flush=True)
    print(f"  torch loop       {spread(a)}", flush=True)
    print(f"  JF_AR_SAMPLER=1  {spread(b)}   ({statistics.median(b) / statistics.median(a):.2f}x)", flush=True)
    llm.exit()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--generate", action="store_true")
    ap.add_argument("--max-tokens", type=int, default=48)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_ar_sampler.py measures on the GPU: none found")
    sampling_part(args.rows, args.iters)
    if args.generate:
        generate_part(args.rows, args.max_tokens)
