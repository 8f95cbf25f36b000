"""``LLMEngine`` — request plumbing with the reference's surface (inference_engine/engine/llm_engine.py:15-202):
``add_request``, ``step``, ``is_finished``, ``generate`` returning ``[{"text", "token_ids"}]``, ``exit``.  A request whose
SamplingParams carries a planted ``logprobs`` (0..20) also gets ``"logprobs"``, ``"ranks"`` and, above 0, ``"top_logprobs"``."""
from __future__ import annotations

import atexit
import copy
import sys
from dataclasses import fields
from time import perf_counter

from ..config import Config
from ..sampling_params import SamplingParams
from .model_runner import ModelRunner
from .scheduler import Scheduler
from .sequence import Sequence, SequenceStatus


class LLMEngine:
    def __init__(self, model, tokenizer_path=None, **kwargs):
        config_fields = {f.name for f in fields(Config)}
        config = Config(model, **{k: v for k, v in kwargs.items() if k in config_fields})       # ENG:20-22
        self.config = config
        self.ps, self.events, self._exited = [], [], False
        self._logprob_outputs = {}                                 # seq_id -> the extra output keys of a finished request that asked
        self.model_runner = ModelRunner(config, 0, self.events, device=kwargs.get("device"))
        self.tokenizer = None
        tok_path = tokenizer_path or model
        if tok_path != "none":
            try:
                from transformers import AutoTokenizer
                self.tokenizer = AutoTokenizer.from_pretrained(tok_path, use_fast=True)
            except Exception as e:  # no tokenizer files: token-id prompts still work
                print(f"[LLMEngine] tokenizer not loaded from {tok_path} ({type(e).__name__}); prompts must be token ids", file=sys.stderr, flush=True)
        if self.tokenizer is not None:
            config.eos = self.tokenizer.eos_token_id
            config.pad = self.tokenizer.pad_token_id if self.tokenizer.pad_token_id is not None else self.tokenizer.eos_token_id
        else:
            config.eos, config.pad = config.hf_config.eos_token_id, config.hf_config.pad_token_id
        self.scheduler = Scheduler(config)
        self.model_runner.block_manager = self.scheduler.block_manager
        self.scheduler.set_kv_cache(self.model_runner.kv_cache)
        self.scheduler.release_row = self.model_runner.release
        atexit.register(self.exit)

    def exit(self):
        if getattr(self, "_exited", False):
            return
        self._exited = True
        if getattr(self, "model_runner", None) is not None:
            self.model_runner.call("exit")
            self.model_runner = None

    def add_request(self, prompt, sampling_params: SamplingParams):
        if isinstance(prompt, str):
            if self.tokenizer is None:
                raise ValueError("string prompts need a tokenizer; pass token ids or a tokenizer_path")
            prompt = self.tokenizer.encode(prompt)
        seq = Sequence(prompt, sampling_params)
        self.scheduler.add(seq)

    def step(self):
        seqs, is_prefill = self.scheduler.schedule()
        result = self.model_runner.call("run", seqs, is_prefill)
        if result is None or (is_prefill and len(result) > 0 and result[0] == []):              # ENG:90-93
            return [], sum(len(seq) for seq in seqs)
        if len(result) > 0 and isinstance(result[0], dict):                                     # on-policy, ENG:95-116
            # every sequence of the batch finishes and carries the WHOLE list of per-sequence records, as in the reference
            num_new = 0 if is_prefill else sum(seq.num_completion_tokens for seq in seqs)
            for seq in seqs:
                seq.status = SequenceStatus.FINISHED
                seq._rollout_records = result
                if seq in self.scheduler.running:
                    self.scheduler.running.remove(seq)
                self.scheduler.block_manager.deallocate(seq)      # (the reference keeps them, ENG:106-110: a second rollout batch then finds the pool smaller)
                self.model_runner.release(seq)
            return [(seq.seq_id, seq._rollout_records) for seq in seqs], (-num_new if num_new > 0 else 0)
        token_ids = result
        is_jacobi = len(token_ids) > 0 and isinstance(token_ids[0], (list, tuple))
        if is_jacobi:
            self.scheduler.postprocess_jacobi(seqs, token_ids)
            num_new = sum(len(t) for t in token_ids)
        else:
            self.scheduler.postprocess(seqs, token_ids)
            num_new = len(seqs)
        outputs = []
        for seq in seqs:
            if seq.is_finished:
                outputs.append((seq.seq_id, seq.completion_token_ids))
                n_top = getattr(getattr(seq, "sampling_params", None), "logprobs", None)
                if n_top is not None:                              # the request asked for log-probabilities (ModelRunner._ar_logprobs)
                    n = seq.num_completion_tokens
                    extra = {"logprobs": list(getattr(seq, "_logprobs", []))[:n], "ranks": list(getattr(seq, "_ranks", []))[:n]}
                    if int(n_top) > 0:
                        extra["top_logprobs"] = list(getattr(seq, "_top_logprobs", []))[:n]
                    self._logprob_outputs[seq.seq_id] = extra
                self.model_runner.release(seq)
        return outputs, (sum(len(seq) for seq in seqs) if is_prefill else -num_new)

    def is_finished(self):
        return self.scheduler.is_finished()

    def generate(self, prompts, sampling_params, use_tqdm: bool = True, logprobs=None):
        """``logprobs`` (not in the reference): an int asks for every request, a list gives one value per prompt (None: that
        request does not ask); it is planted on a copy of the request's SamplingParams.  0: the log-probability and rank of every
        generated token; 1..20: the top N (id, log-probability) pairs as well.  The values are the model's distribution at the
        request's temperature, top_k / top_p not applied (include/jacobiforcing.h: jf_logprobs_rows).  Autoregressive outputs
        gain "logprobs" / "ranks" [/ "top_logprobs"], rollout records "answer_logprobs" [/ "answer_top_logprobs"]."""
        if logprobs is not None:
            lp_list = list(logprobs) if isinstance(logprobs, (list, tuple)) else [logprobs] * len(prompts)
            if len(lp_list) != len(prompts):
                raise ValueError(f"logprobs: {len(lp_list)} values for {len(prompts)} prompts")
            for n in lp_list:
                if n is not None and (isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= 20):
                    raise ValueError(f"logprobs must be None or an int in 0..20, got {n!r}")
            if not isinstance(sampling_params, list):
                sampling_params = [sampling_params] * len(prompts)
            if len(sampling_params) != len(prompts):
                raise ValueError(f"logprobs: {len(sampling_params)} sampling parameters for {len(prompts)} prompts")
            sampling_params = [copy.copy(sp) for sp in sampling_params]
            for sp, n in zip(sampling_params, lp_list):
                if n is not None:
                    sp.logprobs = int(n)
        pbar = None
        if use_tqdm:
            from tqdm.auto import tqdm
            pbar = tqdm(total=len(prompts), desc="Generating", dynamic_ncols=True)
        if not isinstance(sampling_params, list):
            sampling_params = [sampling_params] * len(prompts)
        for prompt, sp in zip(prompts, sampling_params):
            self.add_request(prompt, sp)
        outputs = {}
        prefill_tp = decode_tp = 0.0
        while not self.is_finished():
            t = perf_counter()
            output, num_tokens = self.step()
            if pbar is not None:
                dt = max(perf_counter() - t, 1e-9)
                if num_tokens > 0:
                    prefill_tp = num_tokens / dt
                else:
                    decode_tp = -num_tokens / dt
                pbar.set_postfix({"Prefill": f"{int(prefill_tp)}tok/s", "Decode": f"{int(decode_tp)}tok/s"})
            for seq_id, toks in output:
                outputs[seq_id] = toks
                if pbar is not None:
                    pbar.update(1)
        if pbar is not None:
            pbar.close()
        ordered = [outputs[seq_id] for seq_id in sorted(outputs)]
        if ordered and isinstance(ordered[0], list) and ordered[0] and isinstance(ordered[0][0], dict):   # ENG:176-185
            records = []
            for seq_output in ordered:          # one copy of the batch's record list per sequence (reference behaviour)
                records.extend(seq_output) if isinstance(seq_output, list) else records.append(seq_output)
            return records
        res = []
        for seq_id in sorted(outputs):
            toks = [int(t) for t in outputs[seq_id]]
            text = self.tokenizer.decode(toks) if self.tokenizer is not None else ""
            res.append({"text": text, "token_ids": toks})
            res[-1].update(self._logprob_outputs.pop(seq_id, {}))   # "logprobs", "ranks" [, "top_logprobs"]: only for requests that asked
        return res
