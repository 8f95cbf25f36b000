#!/usr/bin/env python3
"""On-policy rollout records: lock-step (one forward for every open sequence) against the sequential path, same process.

The package's own Qwen2 forward through ``LLM.generate(jacobi_on_policy=True)``: ``--model 7b`` is the bench's random-init
Qwen2.5-Coder-7B shape in bf16 (random weights accept ~1 token per forward: this measures forwards saved, not a checkpoint's
acceptance), ``--model toy`` the trained ``tests/golden/toy_periodic`` checkpoint.  Per batch size: one warm-up of each mode,
then ``--reps`` repetitions alternating the two modes, device events around the whole call (prefill included), median.
Reported: records tokens/s, forwards issued, and for lock-step the mean share of padded rows per forward,
1 - sum R_i / (G * Lm).

    python tools/onpolicy_rollout_bench.py --model 7b --batch 1 8 64 --out profiles/onpolicy_lockstep.txt
"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from jacobiforcing_amd import LLM, SamplingParams  # noqa: E402
from jacobiforcing_amd.synthetic import humaneval_shaped_prompts  # noqa: E402
from jacobiforcing_amd.tuning import enable_tuned_gemms  # noqa: E402


def build_llm(model: str, max_batch: int):
    if model == "toy":
        cfg = json.loads((ROOT / "tests" / "golden" / "toy_periodic" / "config.json").read_text())
        llm = LLM(str(ROOT / "tests" / "golden" / "toy_periodic"), tokenizer_path="none", device="cuda", max_model_len=512,
                  max_num_batched_tokens=max(8192, 512 * max_batch), max_num_seqs=max_batch)
        return llm, int(cfg["vocab_size"]) - 2
    cfg = dict(vocab_size=152064, hidden_size=3584, intermediate_size=18944, num_hidden_layers=28, num_attention_heads=28,
               num_key_value_heads=4, max_position_embeddings=32768, rms_norm_eps=1e-6, rope_theta=1000000.0,
               tie_word_embeddings=False, eos_token_id=-1, pad_token_id=151643, model_type="qwen2")   # no EOS: random weights emit any id
    d = tempfile.mkdtemp()
    (Path(d) / "config.json").write_text(json.dumps(cfg))
    enable_tuned_gemms()
    return LLM(d, tokenizer_path="none", max_model_len=2048, max_num_batched_tokens=65536, max_num_seqs=max_batch), 151643


def one_call(llm, prompts, sp_kw, lockstep: bool):
    sp = SamplingParams(**sp_kw)
    sp.jacobi_lockstep = lockstep                      # planted on the request, like top_k / top_p
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = llm.generate(prompts, sp, use_tqdm=False)
    end.record()
    torch.cuda.synchronize()
    recs = out[:len(prompts)]                           # (generate returns the batch's record list once per sequence)
    last = [r[max(r)] for r in recs if r]
    tokens = sum(int(round(x["tokens_per_forward"] * x["num_forwards"])) for x in last)
    seq_forwards = sum(int(x["num_forwards"]) for x in last)
    dec = llm.model_runner.jacobi_decoder
    fw = list(dec.lockstep_forwards) if lockstep else []
    padded = statistics.fmean(1.0 - v / float(g * lm) for g, lm, v in fw) if fw else 0.0
    return dict(seconds=start.elapsed_time(end) / 1e3, tokens=tokens, forwards=len(fw) if lockstep else seq_forwards, padded=padded)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["7b", "toy"], default="7b")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--block-len", type=int, default=32)
    ap.add_argument("--max-tokens", type=int, default=128)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", default="", help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default="", help="append the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", str(ROOT), "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = "unknown"
    llm, vocab_hi = build_llm(args.model, max(args.batch))
    sp_kw = dict(temperature=args.temperature, max_tokens=args.max_tokens, ignore_eos=True, decode_strategy="jacobi",
                 jacobi_block_len=args.block_len, jacobi_on_policy=True)
    lines = [f"commit {commit}", "command: " + " ".join(["python", "tools/onpolicy_rollout_bench.py"] + sys.argv[1:]),
             f"model {args.model}, block {args.block_len}, max_tokens {args.max_tokens}, T {args.temperature}, "
             f"{args.reps} repetitions (median; min..max in brackets), device events around LLM.generate (prefill included)"
             + (", prompts cut to the toy's 512 positions" if args.model == "toy" else "")]
    for B in args.batch:
        prompts = humaneval_shaped_prompts(B, seed=1234, vocab_hi=vocab_hi)
        if args.model == "toy":                                                    # 512 positions: prompt + budget + one block must fit
            prompts = [p[:512 - args.max_tokens - 2 * args.block_len] for p in prompts]
        runs = {False: [], True: []}
        for mode in (False, True):
            one_call(llm, prompts, sp_kw, mode)                                  # warm-up: code objects, GEMM choices, buffers
        for _ in range(args.reps):
            for mode in (False, True):
                runs[mode].append(one_call(llm, prompts, sp_kw, mode))
        rate = {}
        for mode in (False, True):
            tps = [r["tokens"] / r["seconds"] for r in runs[mode]]
            rate[mode] = statistics.median(tps)
            mid = sorted(runs[mode], key=lambda r: r["tokens"] / r["seconds"])[len(tps) // 2]
            lines.append(f"B={B:3d} lockstep={'on ' if mode else 'off'} {rate[mode]:9.1f} tok/s [{min(tps):.1f}..{max(tps):.1f}]  "
                         f"tokens {mid['tokens']:6d}  forwards {mid['forwards']:6d}  padded rows {100.0 * mid['padded']:5.1f} %")
        lines.append(f"B={B:3d} ratio on/off {rate[True] / rate[False]:.2f}")
        print("\n".join(lines[-3:]), flush=True)
    report = "\n".join(lines) + "\n"
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report)
    print(report)


if __name__ == "__main__":
    main()
