"""Per-token log-probabilities: ``jf_logprobs_rows`` against a float64 numpy reference, ``ops.LogprobRows`` and its routing
through ``ModelRunner._run_autoregressive`` / ``LLM.generate(logprobs=)`` and the on-policy rollout steppers.

The definition under test (include/jacobiforcing.h): with xs the scaled row (JF_F32: fl32(x / T); JF_BF16: bf16(float(x) / float(T));
T == 1 leaves x as it is), m = max xs and S = sum exp(xs - m): logprob(id) = (xs[id] - m) - ln S — the model's distribution at the
request's temperature, top_k / top_p not applied; order = descending xs, equal xs by ascending id; rank = 1 + the ids in front.

Comparison rules: ids and ranks exactly, no case left out; log-probabilities within 1e-4 + 3.5e-7 |m| + 2^-23 |want| (twice the
header's bound on a float32 row sum plus one float32 rounding of the result); -inf and NaN by class."""
import ctypes as C
import fnmatch
import functools
import math
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from jacobiforcing_amd import LLM, SamplingParams
from jacobiforcing_amd import _native as N
from jacobiforcing_amd import ops
from jacobiforcing_amd.engine.model_runner import ModelRunner
from oracle import jacobi_oracle as O

from .backends import _addr, _view, device_for, use_backend
from .test_ar_sampler import _DrawSim, model_dir, planted  # noqa: F401  (model_dir is a fixture)
from .test_onpolicy_lockstep import _build, _fuzz_setup, _planted_batch

ROOT = Path(__file__).resolve().parents[1]
GPU = pytest.mark.gpu
DEV = "cuda:0"
SYMBOLS = ("jf_logprobs_workspace_bytes", "jf_logprobs_rows")
CHUNK = {"f32": 256 * 8 * 4, "bf16": 256 * 8 * 8}                      # elements of a (row, chunk) workgroup (jf_logprobs.hip: LP_TPB * LP_NV * EPV)


# ------------------------------------------------------------------------------------- the reference (float64 numpy)
def scaled_rows(x: np.ndarray, ldt: str, T: float) -> np.ndarray:
    """xs as float32 values: the scaling of include/jacobiforcing.h (a true division, rounded once more to bf16 for bf16 rows)."""
    t = np.float32(1.0 if T <= 0 else T)
    x = np.asarray(x, dtype=np.float32)
    if t == np.float32(1.0):
        return x
    with np.errstate(over="ignore", invalid="ignore"):
        q = (x / t).astype(np.float32)
    return O.bf16_round(q) if ldt == "bf16" else q


class RefRow:
    """One row: logprob [V] float64, rank [V] (-1 on a row without log-probabilities), order [V], m."""

    def __init__(self, xs32: np.ndarray):
        xs = xs32.astype(np.float64)
        V = xs.shape[0]
        ids = np.arange(V)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            self.bad = bool(np.isnan(xs).any() or np.isposinf(xs).any() or not np.isfinite(xs.max()))
            self.order = np.lexsort((ids, -xs))
            self.rank = np.empty(V, dtype=np.int64)
            self.rank[self.order] = np.arange(1, V + 1)
            if self.bad:
                self.m, self.logprob = 0.0, np.full(V, np.nan)
                self.rank[:] = -1
            else:
                self.m = float(xs.max())
                self.logprob = (xs - self.m) - np.log(np.exp(xs - self.m).sum())

    def expect(self, chosen: int, top_n: int):
        V = self.logprob.shape[0]
        ok = 0 <= chosen < V
        lp, rk = (self.logprob[chosen], int(self.rank[chosen])) if ok else (np.nan, -1)
        ids = np.full(top_n, -1, dtype=np.int64)
        tl = np.full(top_n, np.nan if self.bad else -np.inf)
        if not self.bad:
            k = min(top_n, V)
            ids[:k] = self.order[:k]
            tl[:k] = self.logprob[self.order[:k]]
        return float(lp), rk, ids, tl


def reference(x: np.ndarray, ldt: str, T: float):
    return [RefRow(r) for r in scaled_rows(x, ldt, T)]


def close(got, want, m):
    """the comparison rule for log-probabilities (arrays or scalars)"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    nan, ninf = np.isnan(want), np.isneginf(want)
    if not (np.array_equal(np.isnan(got), nan) and np.array_equal(np.isneginf(got), ninf)):
        return False
    fin = ~(nan | ninf)
    with np.errstate(invalid="ignore"):
        err = np.abs(got[fin] - want[fin])
    return bool((err <= 1e-4 + 3.5e-7 * abs(m) + 2.0 ** -23 * np.abs(want[fin])).all())


def check_rows(got, refs, chosen, top_n, what=""):
    lps, ranks, ids, tlp = got
    assert len(lps) == len(ranks) == len(refs) and ids.shape == tlp.shape == (len(refs), top_n)
    for r, (ref, c) in enumerate(zip(refs, chosen)):
        lp, rk, wi, wl = ref.expect(int(c), top_n)
        print(f"{what} row {r} chosen {c}: logprob {lps[r]!r} want {lp!r} rank {ranks[r]} want {rk}")
        assert int(ranks[r]) == rk, (what, r, c, int(ranks[r]), rk)
        assert np.array_equal(ids[r], wi), (what, r, ids[r], wi)
        assert close(lps[r], lp, ref.m), (what, r, c, float(lps[r]), lp)
        assert close(tlp[r], wl, ref.m), (what, r, tlp[r], wl)


def to_dtype(x: np.ndarray, ldt: str) -> np.ndarray:
    return O.bf16_round(x) if ldt == "bf16" else np.asarray(x, dtype=np.float32)


# ------------------------------------------------------------------------------------- the CPU stand-in
class _LpSim(_DrawSim):
    """The CPU stand-in with the new entry points: the reference above on the rows the call points at."""

    def jf_logprobs_workspace_bytes(self, R, V, top_n):
        return 16 if R > 0 and V > 0 else 0

    def jf_logprobs_rows(self, logits, dtype, R, V, stride, temperature, chosen, top_n, logprob, rank, top_ids, top_logprobs, ws,
                         ws_bytes, stream):
        if R <= 0:
            return 0
        refs = reference(self._rows_f32(logits, dtype, R, V, stride), self._ldt(dtype), float(temperature))
        ch = _view(chosen, R, np.int64)
        lp, rk = _view(logprob, R, np.float32), _view(rank, R, np.int32)
        ti = _view(top_ids, R * top_n, np.int64).reshape(R, top_n) if top_n else None
        tl = _view(top_logprobs, R * top_n, np.float32).reshape(R, top_n) if top_n else None
        for r in range(R):
            a, b, c, d = refs[r].expect(int(ch[r]), top_n)
            lp[r], rk[r] = a, b
            if top_n:
                ti[r], tl[r] = c, d
        return 0


class _NoLogprobSymbols:
    """A library whose new entry points are booby-trapped: looking either up fails the test."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        if name in SYMBOLS:
            raise AssertionError(f"a request that did not ask looked up {name}")
        return getattr(self._inner, name)


# ------------------------------------------------------------------------------------- 1. boundary (CPU)
def test_the_entry_points_are_declared_exported_bound_and_counted():
    hdr = (ROOT / "include" / "jacobiforcing.h").read_text()
    assert re.search(r"^JF_API\s+int\s+jf_logprobs_rows\s*\(", hdr, flags=re.M)
    assert re.search(r"^JF_API\s+size_t\s+jf_logprobs_workspace_bytes\s*\(", hdr, flags=re.M)
    assert re.search(r"#define JF_LOGPROBS_MAX_TOP 20\b", hdr) and N.LOGPROBS_MAX_TOP == 20
    emap = (ROOT / "jacobiforcing_amd" / "csrc" / "jf_exports.map").read_text()
    exported_patterns = re.search(r"global:\s*([^;]+);", emap).group(1).split()
    import __graft_entry__ as G
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(G.build_hip())], text=True)
    dynamic = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in SYMBOLS:
        assert any(fnmatch.fnmatchcase(sym, pat) for pat in exported_patterns)
        assert sym in N.EXPORTED_SYMBOLS and sym in dynamic
    assert len(N._SIGNATURES["jf_logprobs_rows"][1]) == 15 and len(N._SIGNATURES["jf_logprobs_workspace_bytes"][1]) == 3
    assert int(re.search(r"#define JF_VERSION (\d+)", hdr).group(1)) == 600          # an addition only
    n_hdr = len(re.findall(r"^JF_API\s", hdr, flags=re.M))
    assert n_hdr == len(N.EXPORTED_SYMBOLS)
    for doc in ("INTEGRATION.md", "COVERAGE.md"):
        assert f"{n_hdr} entry points" in (ROOT / doc).read_text(), doc
    assert "top_k" in hdr[hdr.index("Per-token log-probabilities"):] and "jf_logprobs_rows" in (ROOT / "DESIGN.md").read_text()


# ------------------------------------------------------------------------------------- 2. argument validation (CPU, the real library)
def test_argument_validation_needs_no_gpu():
    """Every JF_E_INVALID path and R == 0 return in front of the first launch: the real library, pointers that are never read."""
    lib = N.load()
    R, V = 2, 64
    need = int(lib.jf_logprobs_workspace_bytes(R, V, 5))
    assert int(lib.jf_logprobs_workspace_bytes(R, V, 20)) > need > int(lib.jf_logprobs_workspace_bytes(R, V, 0)) > 0
    assert lib.jf_logprobs_workspace_bytes(0, V, 5) == 0 and lib.jf_logprobs_workspace_bytes(R, 0, 5) == 0
    fake = C.c_void_p(1 << 20)                                            # 16-byte aligned, never dereferenced
    base = (("logits", fake), ("dtype", N.JF_F32), ("R", R), ("V", V), ("stride", V), ("t", 1.0), ("chosen", fake), ("top_n", 5),
            ("logprob", fake), ("rank", fake), ("top_ids", fake), ("top_lp", fake), ("ws", fake), ("ws_bytes", need), ("stream", None))
    call = lambda **k: lib.jf_logprobs_rows(*[k.get(n, d) for n, d in base])
    assert call(R=0) == N.JF_OK and call(R=-3) == N.JF_OK and call(R=0, logits=None) == N.JF_OK
    for bad in (dict(logits=None), dict(chosen=None), dict(logprob=None), dict(rank=None), dict(ws=None), dict(top_ids=None),
                dict(top_lp=None), dict(dtype=7), dict(V=0), dict(V=1 << 31), dict(stride=V - 1), dict(top_n=-1), dict(top_n=21),
                dict(ws_bytes=need - 1), dict(ws=C.c_void_p((1 << 20) + 8)), dict(R=1 << 31)):
        assert call(**bad) == N.JF_E_INVALID, bad
        assert b"jf_logprobs_rows" in lib.jf_last_error(), bad


# ------------------------------------------------------------------------------------- 3. the reference checks itself (CPU)
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
@pytest.mark.parametrize("T", [1.0, 0.8, 0.3])
def test_reference_agrees_with_torch_on_rows_without_ties(ldt, T):
    rng = np.random.default_rng(5)
    V = 200
    x = to_dtype((rng.permutation(V * 4).reshape(4, V).astype(np.float32) - 400.0) / 16.0, ldt)   # distinct in float32; bf16 may merge some
    xs = scaled_rows(x, ldt, T)
    keep = [r for r in range(4) if len(np.unique(xs[r])) == V]
    if ldt == "f32":
        assert len(keep) == 4
    refs = reference(x, ldt, T)
    for r in range(4):
        want = torch.log_softmax(torch.from_numpy(xs[r].astype(np.float64)), dim=-1)
        assert np.allclose(refs[r].logprob, want.numpy(), rtol=0, atol=1e-12)
        if r in keep:
            tv, ti = torch.topk(want, 20)
            _, _, ids, tl = refs[r].expect(0, 20)
            assert np.array_equal(ids, ti.numpy()) and np.allclose(tl, tv.numpy(), rtol=0, atol=1e-12)
            assert refs[r].rank[int(ti[0])] == 1 and refs[r].rank[int(ti[19])] == 20
    tie = RefRow(np.array([1.0, 3.0, 3.0, -np.inf, 3.0, 0.0, -0.0], dtype=np.float32))
    assert tie.order.tolist() == [1, 2, 4, 0, 5, 6, 3] and tie.rank.tolist() == [4, 1, 2, 7, 3, 5, 6]
    assert tie.expect(3, 9)[0] == -np.inf and np.isnan(tie.expect(7, 0)[0]) and tie.expect(7, 0)[1] == -1    # an id outside the row
    assert tie.expect(-1, 0)[1] == -1 and tie.expect(1, 9)[2].tolist() == [1, 2, 4, 0, 5, 6, 3, -1, -1]
    for bad in ([1.0, np.nan], [np.inf, 0.0], [-np.inf, -np.inf]):
        b = RefRow(np.array(bad, dtype=np.float32))
        assert b.bad and np.isnan(b.expect(0, 2)[0]) and b.expect(0, 2)[1] == -1 and b.expect(0, 2)[2].tolist() == [-1, -1]


# ------------------------------------------------------------------------------------- 4. resources (CPU, cross-compile)
def test_partial_kernels_use_no_scratch():
    """Every instantiation of the streaming kernel keeps its chunk in registers: ScratchSize == 0 (the VGPR counts are printed,
    not pinned)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "jacobiforcing_amd" / "csrc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", f"-I{ROOT / 'include'}", f"-I{csrc}",
                          str(csrc / "jf_logprobs.hip"), "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {"lp_partial_kernel": 0, "lp_finish_kernel": 0}
    for b in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        name = b.split()[0]
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(name, "VGPRs", vgprs, "scratch", scratch, "LDS", lds)
        for k in seen:
            if k in name:
                seen[k] += 1
                assert scratch == 0, (name, vgprs, scratch)
    assert seen == {"lp_partial_kernel": 20, "lp_finish_kernel": 5}         # (2 + 3 scalings) x {vector, element-wise} x {plain, top N}


# ------------------------------------------------------------------------------------- 5. routing (CPU, stand-in library)
def spy_on_logprobs(monkeypatch):
    """Every ``ModelRunner._ar_logprobs`` call as (request ids, their completion lengths at the draw, temperatures, logits rows
    float32 [B, V], their dtype name, the step's tokens)."""
    calls, real = [], ModelRunner._ar_logprobs

    def spy(self, seqs, temps, logits, toks):
        calls.append(([s.seq_id for s in seqs], [s.num_completion_tokens for s in seqs], list(temps),
                      logits.detach().float().cpu().numpy().copy(), "bf16" if logits.dtype == torch.bfloat16 else "f32", list(toks)))
        return real(self, seqs, temps, logits, toks)
    monkeypatch.setattr(ModelRunner, "_ar_logprobs", spy)
    return calls


def expected_lists(calls, seq_id, n_top):
    """The reference on the spied logits for one request: (tokens, logprobs, ranks, top lists, m per token) by completion index
    (a later draw of the same index — a re-prefilled request — replaces the earlier one, as the lists do)."""
    by_j = {}
    for ids, js, temps, rows, ldt, toks in calls:
        if seq_id in ids:
            i = ids.index(seq_id)
            ref = RefRow(scaled_rows(rows[i:i + 1], ldt, temps[i] if temps[i] > 0 else 1.0)[0])
            lp, rk, ti, tl = ref.expect(int(toks[i]), n_top)
            by_j[js[i]] = (int(toks[i]), lp, rk, list(zip(ti.tolist(), tl.tolist())), ref.m)
    assert sorted(by_j) == list(range(len(by_j)))
    return [by_j[j] for j in range(len(by_j))]


def check_output(out, calls, seq_id, n_top):
    want = expected_lists(calls, seq_id, n_top)
    n = len(out["token_ids"])
    assert n and len(out["logprobs"]) == len(out["ranks"]) == n and [w[0] for w in want][:n] == out["token_ids"]
    assert ("top_logprobs" in out) == (n_top > 0)
    for j in range(n):
        tok, lp, rk, top, m = want[j]
        assert out["ranks"][j] == rk and close(out["logprobs"][j], lp, m), (j, out["logprobs"][j], lp)
        assert out["logprobs"][j] <= 0.0 and rk >= 1
        if n_top:
            got = out["top_logprobs"][j]
            assert [g[0] for g in got] == [t[0] for t in top] and close([g[1] for g in got], [t[1] for t in top], m)
            assert (rk <= n_top) == (tok in [g[0] for g in got])                  # rank <= N  <=>  the token sits at top[rank - 1]
            if rk <= n_top:
                assert got[rk - 1][0] == tok and got[rk - 1][1] == out["logprobs"][j]
            assert all(a[1] >= b[1] for a, b in zip(got, got[1:]))


def _llm(model_dir, backend, max_num_seqs=4):
    return LLM(model_dir, tokenizer_path="none", device=device_for(backend), max_model_len=512, max_num_batched_tokens=512,
               max_num_seqs=max_num_seqs)


def _seq_ids(llm, n):
    """the ids the next n requests will get (Sequence.counter is global)"""
    from jacobiforcing_amd.engine.sequence import Sequence
    probe = next(Sequence.counter)
    return list(range(probe + 1, probe + 1 + n))


def run_greedy_and_seeded(model_dir, monkeypatch, backend):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.delenv("JF_AR_SAMPLER", raising=False)
    calls = spy_on_logprobs(monkeypatch)
    with use_backend(backend):
        if backend == "hostsim":
            N._LIB = _LpSim()
        llm = _llm(model_dir, backend)
        prompts = [[5, 9, 200, 31, 7], [100, 101, 102]]
        # greedy: every token is the most likely one
        ids = _seq_ids(llm, 2)
        out = llm.generate(prompts, planted(0.0, 6), logprobs=2, use_tqdm=False)
        for o, sid in zip(out, ids):
            assert sorted(o) == ["logprobs", "ranks", "text", "token_ids", "top_logprobs"]
            check_output(o, calls, sid, 2)
            assert o["ranks"] == [1] * 6 and all(t[0][0] == tok for t, tok in zip(o["top_logprobs"], o["token_ids"]))
        assert all(c[2] == [0.0, 0.0] for c in calls)
        # seeded T = 0.8 (the batched HIP sampler), stopped by max_tokens
        calls.clear()
        ids = _seq_ids(llm, 2)
        out = llm.generate(prompts, planted(0.8, 7, top_k=5), seed=41, logprobs=2, use_tqdm=False)
        for o, sid in zip(out, ids):
            check_output(o, calls, sid, 2)
            assert len(o["token_ids"]) == 7
        assert any(r > 1 for o in out for r in o["ranks"])                        # sampled, not greedy; the values are the UNFILTERED ones
        assert all(c[2] == [0.8, 0.8] for c in calls)
        llm.exit()


def test_generate_returns_logprobs_for_greedy_and_seeded_requests(model_dir, monkeypatch):
    run_greedy_and_seeded(model_dir, monkeypatch, "hostsim")


def test_only_the_requests_that_ask_get_the_keys_and_temperatures_mix(model_dir, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.delenv("JF_AR_SAMPLER", raising=False)
    calls = spy_on_logprobs(monkeypatch)
    with use_backend("hostsim"):
        N._LIB = _LpSim()
        llm = _llm(model_dir, "hostsim")
        prompts = [[5, 9, 200, 31, 7], [100, 101, 102], [250, 3], [7, 7, 7, 7]]
        sps = [planted(0.8, 6), planted(0.0, 5), planted(0.3, 6), planted(0.8, 4)]
        ids = _seq_ids(llm, 4)
        out = llm.generate(prompts, sps, seed=[41, None, 43, 44], logprobs=[3, 0, None, 20], use_tqdm=False)
        assert sorted(out[2]) == ["text", "token_ids"] and sorted(out[1]) == ["logprobs", "ranks", "text", "token_ids"]
        for k, n in ((0, 3), (1, 0), (3, 20)):
            check_output(out[k], calls, ids[k], n)
        assert [len(o["token_ids"]) for o in out] == [6, 5, 6, 4]
        assert not hasattr(sps[0], "logprobs")                             # the caller's objects are not written to
        llm.exit()


def test_eos_and_queued_requests_keep_lists_and_tokens_together(model_dir, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.delenv("JF_AR_SAMPLER", raising=False)
    calls = spy_on_logprobs(monkeypatch)
    with use_backend("hostsim"):
        N._LIB = _LpSim()
        llm = _llm(model_dir, "hostsim", max_num_seqs=2)                   # two cache rows
        prompts = [[5 + i, 9, 200 - i, 31, 7][:3 + i % 3] for i in range(5)]
        sp = planted(0.0, 9)
        ids = _seq_ids(llm, 5)
        together = llm.generate(prompts, sp, logprobs=1, use_tqdm=False)    # five requests: three wait for a row
        for o, sid in zip(together, ids):
            check_output(o, calls, sid, 1)
        alone = [llm.generate([p], sp, logprobs=1, use_tqdm=False)[0] for p in prompts]
        for a, b in zip(together, alone):
            assert a["token_ids"] == b["token_ids"] and a["ranks"] == b["ranks"]
            assert np.allclose(a["logprobs"], b["logprobs"], rtol=0, atol=1e-5)
            assert [[t[0] for t in row] for row in a["top_logprobs"]] == [[t[0] for t in row] for row in b["top_logprobs"]]
        # a request stopped by EOS: its own second token becomes the EOS id of a request that does not ignore it
        eos_run = SamplingParams(temperature=0.0, max_tokens=9, ignore_eos=False)
        stop_tok = together[0]["token_ids"][2]
        monkeypatch.setattr(llm.scheduler, "eos", stop_tok)
        calls.clear()
        sid = _seq_ids(llm, 1)[0]
        o = llm.generate(prompts[:1], eos_run, logprobs=1, use_tqdm=False)[0]
        assert o["token_ids"] == together[0]["token_ids"][:o["token_ids"].index(stop_tok) + 1] and len(o["token_ids"]) < 9
        check_output(o, calls, sid, 1)
        llm.exit()


def test_requests_that_do_not_ask_never_touch_the_new_symbols(model_dir, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.delenv("JF_AR_SAMPLER", raising=False)

    def no_rows(*a, **k):
        raise AssertionError("LogprobRows was constructed for requests that did not ask")
    monkeypatch.setattr(ops, "LogprobRows", no_rows)
    with use_backend("hostsim"):
        N._LIB = _NoLogprobSymbols(_LpSim())
        with pytest.raises(AssertionError):
            N.lib().jf_logprobs_rows
        llm = _llm(model_dir, "hostsim")
        out = llm.generate([[5, 9, 200, 31, 7], [100, 101, 102], [250, 3]], [planted(0.8, 6, top_k=5), planted(1.0, 6), planted(0.0, 6)],
                           seed=[41, None, None], use_tqdm=False)
        assert all(sorted(o) == ["text", "token_ids"] and len(o["token_ids"]) == 6 for o in out)
        assert llm.model_runner._logprob_rows is None
        llm.exit()


def test_bad_values_and_the_strategies_without_logprobs_raise(model_dir, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    with use_backend("hostsim"):
        N._LIB = _LpSim()
        llm = _llm(model_dir, "hostsim")
        prompts = [[5, 9, 200], [100, 101, 102]]
        for bad in (21, -1, [1], [1, 2, 3], 1.5, [0, 21]):
            with pytest.raises(ValueError):
                llm.generate(prompts, planted(0.0, 4), logprobs=bad, use_tqdm=False)
        assert not llm.scheduler.waiting and not llm.scheduler.running          # nothing was queued by the refused calls
        with pytest.raises(NotImplementedError, match="follow-up"):
            llm.generate(prompts, SamplingParams(temperature=0.0, max_tokens=8, decode_strategy="jacobi", jacobi_block_len=4),
                         logprobs=1, use_tqdm=False)
        llm.exit()
        llm = _llm(model_dir, "hostsim")
        with pytest.raises(NotImplementedError, match="follow-up"):
            llm.generate(prompts, SamplingParams(temperature=0.0, max_tokens=8), logprobs=0, jacobi_num_blocks=2, jacobi_block_len=4,
                         use_tqdm=False)
        llm.exit()


# ------------------------------------------------------------------------------------- 6. rollouts (CPU, stand-in library)
def spy_on_steppers(monkeypatch):
    """Every stepper ``step`` that was asked for log-probabilities: (logits float32 [rows, V], dtype name, temperature, committed
    lists, the returned (logprobs, top_ids, top_logprobs) per sequence, top_n)."""
    calls = []
    real_b, real_s = ops.OnPolicyBatchStepper.step, ops.OnPolicyStepper.step

    def note(logits, temperature, cms, lps, top_n):
        ldt = "bf16" if logits.dtype == torch.bfloat16 else "f32"
        calls.append((logits.detach().float().cpu().numpy().copy(), ldt, float(temperature), cms, lps, top_n))

    def step_b(self, proposed, n_rows, logits, temperature, seq_index, top_k=0, top_p=0.0, **kw):
        res = real_b(self, proposed, n_rows, logits, temperature, seq_index, top_k, top_p, **kw)
        if kw.get("logprobs") is not None:
            note(logits, temperature, res[1], res[3], kw["top_n"])
        return res

    def step_s(self, proposed, logits, temperature, cursors, top_k=0, top_p=0.0, **kw):
        res = real_s(self, proposed, logits, temperature, cursors, top_k, top_p, **kw)
        if kw.get("logprobs") is not None:
            note(logits[None], temperature, [res[1]], [res[3]], kw["top_n"])
        return res
    monkeypatch.setattr(ops.OnPolicyBatchStepper, "step", step_b)
    monkeypatch.setattr(ops.OnPolicyStepper, "step", step_s)
    return calls


def check_stepper_calls(calls):
    """every committed token's values equal the reference on the logits that step saw"""
    n = 0
    for logits, ldt, T, cms, lps, top_n in calls:
        G, Lm, V = logits.shape
        for g in range(G):
            refs = reference(logits[g, :len(cms[g])], ldt, T)
            got = (lps[g][0][:len(cms[g])], np.array([refs[t].expect(c, 0)[1] for t, c in enumerate(cms[g])]),
                   lps[g][1][:len(cms[g])], lps[g][2][:len(cms[g])])
            check_rows(got, refs, cms[g], top_n)
            n += len(cms[g])
    return n


def kept_tokens(record):
    """tokens every block of one sequence's record appended and kept: the growth of the prefix from block to block"""
    ks = sorted(record)
    lens = [len(record[k]["prompt_ids"]) for k in ks] + [len(record[ks[-1]]["teacher_output_ids"])]
    return [b - a for a, b in zip(lens, lens[1:])]


def strip(records):
    return [{k: {key: v for key, v in blk.items() if key not in ("answer_logprobs", "answer_top_logprobs")} for k, blk in rec.items()}
            for rec in records]


def run_rollouts(cfg, backend, asks, lockstep, only=None):
    """the fuzz batch of tests/test_onpolicy_lockstep.py with ``logprobs`` planted per request (None: it does not ask)"""
    with use_backend(backend):
        if backend == "hostsim":
            N._LIB = _LpSim()
        H, dec, seqs, models = _build(cfg, backend)
        for s, n in zip(seqs, asks):
            if n is not None:
                s.sampling_params.logprobs = n
        items = cfg["items"]
        if lockstep:
            dec.set_streams_per_sequence([O.ScriptedRandom(O.CounterStream(9000 + it["seed"])) for it in items],
                                         [it["unis"] for it in items], [it["multi"] for it in items])
            return dec.generate_rollout_records_batch(seqs, lockstep=True)
        out = []
        for i, it in enumerate(items):                                    # the sequential path: every sequence alone with its streams
            dec.set_streams(O.ScriptedRandom(O.CounterStream(9000 + it["seed"])), it["unis"], it["multi"])
            rec = dec.generate_rollout_records_batch([seqs[i]])[0]
            for blk in rec.values():
                blk["data_id"] = f"data_{i}"
            out.append(rec)
        return out


@pytest.mark.parametrize("seed", [3, 6, 13, 22])
def test_rollout_records_carry_the_logprobs_of_the_kept_tokens(seed, monkeypatch):
    cfg = _fuzz_setup(seed)
    B = len(cfg["items"])
    asks = [(2, 0, None, 5)[i % 4] for i in range(B)]
    plain = run_rollouts(cfg, "hostsim", [None] * B, lockstep=True)
    calls = spy_on_steppers(monkeypatch)
    lock = run_rollouts(cfg, "hostsim", asks, lockstep=True)
    n_lock = check_stepper_calls(calls)
    calls.clear()
    seq = run_rollouts(cfg, "hostsim", asks, lockstep=False)
    n_seq = check_stepper_calls(calls)
    assert n_lock > 0 and n_seq > 0
    for i in range(B):
        for k in lock[i]:
            lock[i][k]["teacher_output_ids"] = seq[i][k]["teacher_output_ids"] = list(lock[i][k]["teacher_output_ids"])
    assert strip(lock) == plain                                           # without the new keys: the records of a run that did not ask
    assert strip(seq) == strip(lock)
    for i, n in enumerate(asks):
        kept = kept_tokens(lock[i])
        for k, cnt in zip(sorted(lock[i]), kept):
            blk, sblk = lock[i][k], seq[i][k]
            if n is None:
                assert "answer_logprobs" not in blk and "answer_top_logprobs" not in blk
                continue
            assert len(blk["answer_logprobs"]) == cnt, (i, k, len(blk["answer_logprobs"]), cnt)
            assert all(math.isfinite(v) and v <= 0.0 for v in blk["answer_logprobs"])
            assert blk["answer_logprobs"] == sblk["answer_logprobs"]       # lock-step and sequential: the same values
            assert ("answer_top_logprobs" in blk) == (n > 0)
            if n:
                assert blk["answer_top_logprobs"] == sblk["answer_top_logprobs"]
                assert len(blk["answer_top_logprobs"]) == cnt and all(len(t) == n for t in blk["answer_top_logprobs"])


def test_a_block_closed_by_a_stop_token_keeps_one_logprob_per_kept_token(monkeypatch):
    """Among the fuzz batches: a sequence that ends on a stop id committed in the middle of a step's tokens."""
    hit = 0
    for seed in (3, 6, 13, 22):
        cfg = _fuzz_setup(seed)
        B = len(cfg["items"])
        recs = run_rollouts(cfg, "hostsim", [0] * B, lockstep=True)
        for rec in recs:
            last = rec[max(rec)]
            if last["teacher_output_ids"] and last["teacher_output_ids"][-1] in cfg["stop_ids"]:
                hit += 1
            assert [len(rec[k]["answer_logprobs"]) for k in sorted(rec)] == kept_tokens(rec)
    assert hit > 0


# ------------------------------------------------------------------------------------- 7. kernel vs reference (GPU)
def gpu_rows(x: np.ndarray, ldt: str, pad: int = 0) -> torch.Tensor:
    """The rows on the device in their dtype; pad > 0: a view with row_stride = V + pad into a buffer of NaNs."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16 if ldt == "bf16" else torch.float32)
    if not pad:
        return t.to(DEV)
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)[:, :t.shape[1]]


def gpu_logprobs(lg: torch.Tensor, chosen, T: float, top_n: int, device_chosen: bool = False):
    lp = ops.LogprobRows(DEV, lg.shape[0])
    ch = torch.tensor([int(c) for c in chosen], dtype=torch.int64, device=DEV) if device_chosen else list(chosen)
    lp.run(lg, ch, T, top_n)
    return lp.fetch(lg.shape[0])


@functools.lru_cache(maxsize=None)
def kernel_case(V: int, ldt: str, T: float, scale: float = 2.5):
    """65 random rows in their dtype and their reference (shared by every R / top_n / stride of the shape)."""
    rng = np.random.default_rng([V, ldt == "bf16", int(T * 10), int(scale * 10)])
    x = to_dtype((rng.standard_normal((65, V)) * scale).astype(np.float32), ldt)
    return x, reference(x, ldt, T)


def chosen_kinds(refs, V: int):
    """row by row: the argmax, the last id of the order (rank V), id 0, id V - 1, an id >= V, a negative id, a huge id"""
    kinds = [lambda r: int(r.order[0]), lambda r: int(r.order[-1]), lambda r: 0, lambda r: V - 1, lambda r: V, lambda r: -1,
             lambda r: (1 << 40) + 3]
    return [kinds[i % len(kinds)](r) for i, r in enumerate(refs)]


VS = [1, 2, 63, 64, 65, 257, 4099, CHUNK["f32"] - 1, CHUNK["f32"] + 1, CHUNK["bf16"] - 1, CHUNK["bf16"] + 1]


@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
@pytest.mark.parametrize("V", VS)
def test_kernel_matches_the_reference(V, ldt):
    """Every V with R in {1, 3, 65}, T in {1, 0.8, 0.3}, top_n in {0, 1, 5, 20} (top_n > V included) and the three row strides:
    V (the vector path where V allows), V + 1 (bf16 rows on 2-byte boundaries: the element-wise path) and V + 8."""
    i = 0
    for T in (1.0, 0.8, 0.3):
        x, refs = kernel_case(V, ldt, T)
        chosen = chosen_kinds(refs, V)
        ranks = [refs[r].expect(c, 0)[1] for r, c in enumerate(chosen)]
        assert ranks[0] == 1 and ranks[1] == V and ranks[4] == ranks[5] == ranks[6] == -1
        for R in (1, 3, 65):
            for top_n in (0, 1, 5, 20):
                for pad in (0, 1, 8):
                    i += 1
                    if R == 65 and (i % 3) and V > 300:                    # the large shapes: every third combination at 65 rows
                        continue
                    lg = gpu_rows(x[:R], ldt, pad)
                    assert lg.stride(0) == V + pad or R == 1
                    got = gpu_logprobs(lg, chosen[:R], T, top_n, device_chosen=bool(i % 2))
                    check_rows(got, refs[:R], chosen[:R], top_n, f"V={V} {ldt} T={T} R={R} N={top_n} pad={pad}")


# ------------------------------------------------------------------------------------- 8. order under ties (GPU)
@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
def test_order_under_ties(ldt):
    ch = CHUNK[ldt]
    V = 3 * ch + 77                                                       # four chunks
    rng = np.random.default_rng(8)
    rows = []
    rows.append(np.full(V, 1.5, dtype=np.float32))                        # all equal: top = 0 .. N-1, rank(id) = id + 1
    a = (rng.standard_normal(V) * 2).astype(np.float32)
    a[[ch - 1, ch]] = 30.0                                                # equal maxima: the last id of one chunk, the first of the next
    rows.append(a)
    b = (rng.standard_normal(V) * 2).astype(np.float32)
    b[[0, V - 1]] = 30.0                                                  # ... and at ids 0 and V - 1
    rows.append(b)
    c = (rng.standard_normal(V) * 2).astype(np.float32)
    c[rng.choice(V, 90, replace=False)] = 30.0                            # more than N copies of the maximum, in every chunk
    c[[5, ch + 5, 2 * ch + 5, 3 * ch + 5]] = 30.0
    rows.append(c)
    d = np.zeros(V, dtype=np.float32)
    d[::2] = -0.0                                                         # the two zeros tie
    rows.append(d)
    e = np.full(V, -3.0, dtype=np.float32)
    e[2048 * np.arange(V // 2048)] = 7.0                                  # equal maxima a vector apart ...
    e[:64] = 7.0                                                          # ... and a run of them in the elements of a few threads
    rows.append(e)
    x = to_dtype(np.stack(rows), ldt)
    for T in (1.0, 0.3):
        refs = reference(x, ldt, T)
        assert refs[0].order[:20].tolist() == list(range(20))
        for chosen in ([V - 1, ch, V - 1, 3 * ch + 5, 1, 63], [17, ch - 1, 0, 5, V - 2, 2048]):
            for top_n in (0, 20, 5):
                got = gpu_logprobs(gpu_rows(x, ldt), chosen, T, top_n)
                check_rows(got, refs, chosen, top_n, f"ties {ldt} T={T} N={top_n}")
        assert refs[0].expect(V - 1, 0)[1] == V and refs[1].expect(ch, 0)[1] == 2
    # bf16 rows at T = 0.3 carry exact ties inside their top 20 without planting
    if ldt == "bf16":
        x, refs = kernel_case(152064, "bf16", 0.3, 4.0)
        x, refs = x[:3], refs[:3]
        xs = scaled_rows(x, "bf16", 0.3)
        assert all(len(np.unique(xs[r][refs[r].order[:20]])) < 20 for r in range(3))
        chosen = [int(refs[r].order[19]) for r in range(3)]
        check_rows(gpu_logprobs(gpu_rows(x, ldt), chosen, 0.3, 20), refs, chosen, 20, "bf16 T=0.3 natural ties")


# ------------------------------------------------------------------------------------- 9. special values (GPU)
@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
def test_special_values_and_row_independence(ldt):
    ch = CHUNK[ldt]
    V = ch + 300
    rng = np.random.default_rng(9)
    x = to_dtype((rng.standard_normal((9, V)) * 2.5).astype(np.float32), ldt)
    x[0, rng.random(V) < 0.3] = -np.inf                                   # ids without mass; chosen -inf -> -inf
    x[0, 11] = -np.inf
    x[1, :] = -np.inf                                                     # fewer than N finite ids
    x[1, [3, ch + 2, V - 1]] = [1.0, 2.0, 1.0]
    x[2, :] = -np.inf                                                     # no finite maximum
    x[4, ch + 7] = np.nan
    x[6, 5] = np.inf
    x[7, :ch] = -np.inf                                                   # a whole chunk without mass in a valid row
    refs = reference(x, ldt, 0.8)
    chosen = [11, 3, 0, int(refs[3].order[0]), 9, int(refs[5].order[-1]), 5, ch + 1, 0]
    assert refs[2].bad and refs[4].bad and refs[6].bad and not refs[0].bad and not refs[1].bad and not refs[7].bad
    assert refs[0].expect(11, 0)[0] == -np.inf and refs[1].expect(3, 5)[2].tolist()[:3] == [ch + 2, 3, V - 1]
    lg = gpu_rows(x, ldt)
    for top_n in (0, 5, 20):
        got = gpu_logprobs(lg, chosen, 0.8, top_n)
        check_rows(got, refs, chosen, top_n, f"special {ldt} N={top_n}")
        # the normal rows are bit-identical to a call without the others
        good = [0, 1, 3, 5, 7, 8]
        sub = gpu_logprobs(gpu_rows(x[good], ldt), [chosen[r] for r in good], 0.8, top_n)
        for a, b in zip(got, sub):
            assert np.array_equal(a[good].view(np.uint8), b.view(np.uint8))
        # a row permutation permutes the outputs
        perm = rng.permutation(9)
        pg = gpu_logprobs(gpu_rows(x[perm], ldt), [chosen[r] for r in perm], 0.8, top_n)
        for a, b in zip(got, pg):
            assert np.array_equal(a[perm].view(np.uint8), b.view(np.uint8))
    # an overflowing scaling: x / T = +inf makes the row one without log-probabilities; T <= 0 is T = 1
    y = to_dtype(np.array([[3.0e38, 1.0, 2.0], [1.0, 2.0, 3.0]], dtype=np.float32), ldt)
    check_rows(gpu_logprobs(gpu_rows(y, ldt), [1, 2], 0.3, 2), reference(y, ldt, 0.3), [1, 2], 2, "overflow")
    assert reference(y, ldt, 0.3)[0].bad
    check_rows(gpu_logprobs(gpu_rows(y, ldt), [1, 2], 0.0, 2), reference(y, ldt, 1.0), [1, 2], 2, "T = 0")


# ------------------------------------------------------------------------------------- 10. the real width (GPU)
@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
def test_the_real_vocabulary_against_the_numpy_reference(ldt):
    V = 152064
    for T, scale in ((0.8, 4.0), (1.0, 12.0)):
        x, refs = kernel_case(V, ldt, T, scale)
        chosen = chosen_kinds(refs, V)
        check_rows(gpu_logprobs(gpu_rows(x, ldt), chosen, T, 20), refs, chosen, 20, f"V={V} {ldt} T={T}")


@GPU
def test_64_by_31_bf16_rows_against_torch_on_the_device():
    """The bench's non-greedy shape: torch.log_softmax(x.double()) and a stable descending sort on the device as a second
    reference, with the same rules."""
    R, V, T, Nt = 64 * 31, 152064, 0.8, 20
    g = torch.Generator(device=DEV).manual_seed(10)
    x = (torch.randn((R, V), generator=g, device=DEV) * 4.0).to(torch.bfloat16)
    chosen = torch.randint(0, V, (R,), generator=g, device=DEV)
    chosen[::7] = torch.argmax(x[::7].float(), dim=-1)
    lp = ops.LogprobRows(DEV, R)
    lp.run(x, chosen, T, Nt)
    lps, ranks, ids, tlp = lp.fetch(R)
    ch = chosen.cpu().numpy()
    for a in range(0, R, 248):                                            # slabs of rows: the float64 copy of all of them is 2.4 GB
        xs = (x[a:a + 248].float() / T).to(torch.bfloat16).double()
        want = torch.log_softmax(xs, dim=-1)
        order = torch.sort(xs, dim=-1, descending=True, stable=True).indices
        n = xs.shape[0]
        m = xs.max(dim=-1).values.cpu().numpy()
        rk = (order == chosen[a:a + n, None]).nonzero()[:, 1].cpu().numpy() + 1
        assert np.array_equal(ranks[a:a + n], rk)
        assert np.array_equal(ids[a:a + n], order[:, :Nt].cpu().numpy())
        wl = want.gather(1, chosen[a:a + n, None])[:, 0].cpu().numpy()
        wt = want.gather(1, order[:, :Nt]).cpu().numpy()
        for r in range(n):
            assert close(lps[a + r], wl[r], m[r]) and close(tlp[a + r], wt[r], m[r]), (a + r, lps[a + r], wl[r])
    assert (ranks[::7] == 1).all() and len(np.unique(ch)) > 1000


# ------------------------------------------------------------------------------------- 11. end to end on the GPU
@GPU
def test_generate_returns_logprobs_on_the_gpu(model_dir, monkeypatch):
    run_greedy_and_seeded(model_dir, monkeypatch, "hip")


@GPU
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_lockstep_step_returns_logprobs_at_the_real_vocabulary(dtype):
    """The ragged [4, 12] rectangle of tests/test_onpolicy_lockstep.py at V = 152064: the step's fourth value against the
    reference on the same logits, and the step's own results unchanged by asking."""
    b = _planted_batch(dtype)
    T = 0.7
    with use_backend("hip"):
        def step(**kw):
            st = ops.OnPolicyBatchStepper(b["G"], 16, DEV, b["us"], b["ms"], [b["stop"]])
            st.cursors.copy_(torch.tensor(b["cur0"], dtype=torch.int64))
            return st.step(b["proposed"].to(DEV), b["n_rows"], b["logits"].to(DEV), T, list(range(b["G"])), **kw)
        plain = step()
        rows, cm, rd, lps = step(logprobs=ops.LogprobRows(DEV, 8), top_n=5)
        assert (rows, cm) == plain[:2] and [r["n_committed"] for r in rows] == [12, 1, 1, 5]
        ldt = "bf16" if dtype == torch.bfloat16 else "f32"
        lg = b["logits"].float().numpy()
        for g in range(b["G"]):
            n = len(cm[g])
            refs = reference(lg[g, :n], ldt, T)
            assert lps[g][0].shape == (b["n_rows"][g],) and lps[g][1].shape == (b["n_rows"][g], 5)
            got = (lps[g][0][:n], np.array([refs[t].expect(c, 0)[1] for t, c in enumerate(cm[g])]), lps[g][1][:n], lps[g][2][:n])
            check_rows(got, refs, cm[g], 5, f"lock-step {ldt} sequence {g}")
