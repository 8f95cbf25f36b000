"""The batched sampler of autoregressive requests: jf_rs_draw_rows against the oracle token for token, the per-request
counter-based streams, ``ops.ARSampler`` and its routing through ``ModelRunner._run_autoregressive`` / ``LLM.generate(seed=)``.

The definition under test (include/jacobiforcing.h): tokens[r] = inverse_cdf_sample(target_probs(logits[r], T, dtype, top_k,
top_p), u[r]).  bf16 rows are compared without exception (their float64 sums are exact: sums of 8-bit mantissas whose
exponents span far less than 45 bits at the shapes used here).  On float32 rows the oracle's sequential cumsum and the
kernels' hierarchical sums may differ in the last bits of a float64, so a case whose u * total lies within 1e-9 * total of a
CDF boundary may be left out; the inputs are chosen here, on the CPU, so that at most 1 % of a test's cases are."""
import ctypes as C
import fnmatch
import functools
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from jacobiforcing_amd import LLM, SamplingParams
from jacobiforcing_amd import _native as N
from jacobiforcing_amd import ops
from jacobiforcing_amd.engine.llm_engine import LLMEngine
from oracle import jacobi_oracle as O

from .backends import HostSimLib, _view, device_for, use_backend

ROOT = Path(__file__).resolve().parents[1]
GPU = pytest.mark.gpu
DEV = "cuda:0"
U_MAX = float(np.nextafter(np.float32(1.0), np.float32(0.0)))        # the largest float32 below 1
SYMBOLS = ("jf_rs_draw_workspace_bytes", "jf_rs_draw_rows")


# ------------------------------------------------------------------------------------- 1. boundary (CPU)
def test_the_entry_point_is_declared_exported_and_bound():
    hdr = (ROOT / "include" / "jacobiforcing.h").read_text()
    assert re.search(r"^JF_API\s+int\s+jf_rs_draw_rows\s*\(", hdr, flags=re.M)
    assert re.search(r"^JF_API\s+size_t\s+jf_rs_draw_workspace_bytes\s*\(", hdr, flags=re.M)
    emap = (ROOT / "jacobiforcing_amd" / "csrc" / "jf_exports.map").read_text()
    exported_patterns = re.search(r"global:\s*([^;]+);", emap).group(1).split()
    import __graft_entry__ as G
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(G.build_hip())], text=True)
    dynamic = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for sym in SYMBOLS:
        assert any(fnmatch.fnmatchcase(sym, pat) for pat in exported_patterns)
        assert sym in N.EXPORTED_SYMBOLS and sym in dynamic
    assert len(N._SIGNATURES["jf_rs_draw_rows"][1]) == 14                # the header's argument list
    assert int(re.search(r"#define JF_VERSION (\d+)", hdr).group(1)) == 600   # an addition only


# ------------------------------------------------------------------------------------- 2. the stream (CPU)
def test_stream_is_a_function_of_seed_and_index():
    whole = ops.ar_stream(1234, 0, 1500)
    assert whole.dtype == np.float32 and whole.shape == (1500,)
    k = np.round(whole.astype(np.float64) * 2.0 ** 24)
    assert (whole >= 0).all() and (whole < 1).all() and np.array_equal(k * 2.0 ** -24, whole.astype(np.float64))   # 24-bit uniforms
    assert 0.45 < whole.mean() < 0.55 and len(np.unique(whole)) > 1400
    for block in (1, 3, 4, 5, 64, 256, 1000):                            # any block size
        parts = [ops.ar_stream(1234, s, min(block, 1500 - s)) for s in range(0, 1500, block)]
        assert np.array_equal(np.concatenate(parts), whole), block
    rng = np.random.default_rng(0)
    for j in rng.permutation(1500)[:200]:                                # any order, one at a time
        assert ops.ar_stream(1234, int(j), 1)[0] == whole[j]
    raw = np.random.Philox(key=1234).random_raw(8)                       # the documented construction
    assert np.array_equal(whole[:8], ((raw >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).astype(np.float32))
    assert not np.array_equal(ops.ar_stream(1235, 0, 64), whole[:64])
    assert not np.array_equal(ops.ar_stream(-1, 0, 64), ops.ar_stream(1, 0, 64))
    assert ops.ar_stream(7, 5, 0).shape == (0,)
    with pytest.raises(ValueError):
        ops.ar_stream(7, -1, 4)


class _DrawSim(HostSimLib):
    """The CPU stand-in with the new entry point: the oracle's inverse CDF on the distribution the two stand-in calls in
    front of it define (jf_rs_probs / jf_rs_filter of tests/backends.py)."""

    def jf_rs_draw_workspace_bytes(self, R):
        return self.jf_rs_step_workspace_bytes(R)

    def jf_rs_draw_rows(self, logits, dtype, R, V, stride, row_max, row_sumexp, temperature, filt, u, tokens, ws, ws_bytes, stream):
        probs = self._probs_of(logits, dtype, R, V, stride, temperature, filt)
        uu, out = _view(u, R, np.float32), _view(tokens, R, np.int64)
        for r in range(R):
            out[r] = O.inverse_cdf_sample(probs[r], float(uu[r]))
        return 0


class _NoDrawSymbols:
    """A library whose new entry points are booby-trapped: looking either up fails the test."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        if name in SYMBOLS:
            raise AssertionError(f"an unseeded request looked up {name}")
        return getattr(self._inner, name)


def test_sampler_cache_serves_the_stream():
    with use_backend("hostsim"):
        N._LIB = _DrawSim()
        smp = ops.ARSampler("cpu", 4)
        want = ops.ar_stream(99, 0, 3 * ops.AR_STREAM_BLOCK)
        for j in (700, 0, 255, 256, 1, 699):
            assert smp.uniform(99, j) == want[j]
        assert smp.uniform(100, 5) == ops.ar_stream(100, 5, 1)[0]


# ------------------------------------------------------------------------------------- 3. routing (CPU, stand-in library)
@pytest.fixture()
def model_dir(tmp_path):
    cfg = dict(vocab_size=320, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
               num_key_value_heads=2, max_position_embeddings=1024, rms_norm_eps=1e-6, rope_theta=10000.0,
               tie_word_embeddings=False, eos_token_id=319, pad_token_id=318, model_type="qwen2")
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    return str(tmp_path)


def planted(temperature, max_tokens, **attrs):
    sp = SamplingParams(temperature=temperature, max_tokens=max_tokens, ignore_eos=True)
    for k, v in attrs.items():
        setattr(sp, k, v)
    return sp


def spy_on_sampler(monkeypatch):
    """Every ``ARSampler.sample`` call as (logits rows float32 [B, V], their dtype name, settings, u, tokens)."""
    calls, real = [], ops.ARSampler.sample

    def sample(self, logits, settings, u):
        toks = real(self, logits, settings, u)
        calls.append((logits.detach().float().cpu().numpy().copy(), "bf16" if logits.dtype == torch.bfloat16 else "f32",
                      [tuple(s) for s in settings], np.asarray(u, dtype=np.float32).copy(), list(toks)))
        return toks
    monkeypatch.setattr(ops.ARSampler, "sample", sample)
    return calls


def oracle_token(row, ldt, setting, u):
    t, k, p = setting
    if t == 0.0:
        return int(O.argmax_rows(row[None])[0])
    return O.inverse_cdf_sample(O.target_probs(row[None], t, ldt, k or None, p or None)[0], float(u))


def check_calls(calls, seed_of_setting, n_tokens):
    """Every recorded token is the oracle's on the recorded logits; the j-th draw of the request with a given (distinct)
    setting used uniform j of that request's stream.  Returns the tokens per setting."""
    seen = {s: [] for s in seed_of_setting}
    for rows, ldt, settings, u, toks in calls:
        assert len(settings) == len(set(settings)) == len(toks)           # the requests of these tests have distinct settings
        for r, s in enumerate(settings):
            if s[0] > 0.0:
                j = len(seen[s])
                assert u[r] == ops.ar_stream(seed_of_setting[s], j, 1)[0], (s, j)
            assert toks[r] == oracle_token(rows[r], ldt, s, u[r]), (s, len(seen[s]))
            seen[s].append(toks[r])
    assert all(len(v) == n_tokens for v in seen.values()), {s: len(v) for s, v in seen.items()}
    return seen


def test_seeded_rows_reach_the_sampler_with_their_uniforms_and_settings(model_dir, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.delenv("JF_AR_SAMPLER", raising=False)
    calls = spy_on_sampler(monkeypatch)
    with use_backend("hostsim"):
        N._LIB = _DrawSim()
        llm = LLM(model_dir, tokenizer_path="none", device="cpu", max_model_len=512, max_num_batched_tokens=512, max_num_seqs=4)
        n = 6
        sps = [planted(0.8, n, top_k=5), planted(0.7, n), planted(0.0, n), planted(1.0, n, top_p=0.9)]
        torch.manual_seed(3)
        out = llm.generate([[5, 9, 200, 31, 7], [100, 101, 102], [250, 3], [7, 7, 7, 7]], sps, seed=[41, 42, None, None], use_tqdm=False)
        assert llm.model_runner._ar_sampler is not None
        seen = check_calls(calls, {(0.8, 5, 0.0): 41, (0.7, 0, 0.0): 42, (0.0, 0, 0.0): None}, n)
        assert out[0]["token_ids"] == seen[(0.8, 5, 0.0)] and out[1]["token_ids"] == seen[(0.7, 0, 0.0)]
        assert out[2]["token_ids"] == seen[(0.0, 0, 0.0)]                  # the greedy row rode along
        assert len(out[3]["token_ids"]) == n                              # the unseeded row: torch's loop, in the same steps
        assert all(len(c[2]) == 3 for c in calls)
        # the same seeds alone, in another order: the same tokens
        calls.clear()
        again = llm.generate([[100, 101, 102], [5, 9, 200, 31, 7]], [sps[1], sps[0]], seed=[42, 41], use_tqdm=False)
        assert again[0]["token_ids"] == out[1]["token_ids"] and again[1]["token_ids"] == out[0]["token_ids"]
        llm.exit()


def test_opt_in_variable_seeds_unseeded_requests_once_from_the_global_generator(model_dir, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.setenv("JF_AR_SAMPLER", "1")
    calls = spy_on_sampler(monkeypatch)
    with use_backend("hostsim"):
        N._LIB = _DrawSim()
        llm = LLM(model_dir, tokenizer_path="none", device="cpu", max_model_len=512, max_num_batched_tokens=512, max_num_seqs=4)
        torch.manual_seed(11)
        want = [int(torch.randint(0, 1 << 62, (1,)).item()) for _ in range(2)]     # one draw per request, at its first token
        torch.manual_seed(11)
        n = 5
        out = llm.generate([[5, 9, 200], [100, 101, 102, 103]], [planted(0.9, n), planted(0.6, n, top_k=7)], use_tqdm=False)
        seen = check_calls(calls, {(0.9, 0, 0.0): want[0], (0.6, 7, 0.0): want[1]}, n)
        assert [o["token_ids"] for o in out] == [seen[(0.9, 0, 0.0)], seen[(0.6, 7, 0.0)]]
        llm.exit()


def test_unseeded_requests_never_touch_the_sampler(model_dir, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.delenv("JF_AR_SAMPLER", raising=False)

    def no_sampler(*a, **k):
        raise AssertionError("ARSampler was constructed for an unseeded request")
    monkeypatch.setattr(ops, "ARSampler", no_sampler)
    with use_backend("hostsim"):
        N._LIB = _NoDrawSymbols(_DrawSim())
        with pytest.raises(AssertionError):
            N.lib().jf_rs_draw_rows
        llm = LLM(model_dir, tokenizer_path="none", device="cpu", max_model_len=512, max_num_batched_tokens=512, max_num_seqs=4)
        prompts, sps = [[5, 9, 200, 31, 7], [100, 101, 102], [250, 3]], [planted(0.8, 8, top_k=5), planted(1.0, 8), planted(0.0, 8)]
        torch.manual_seed(5)
        a = llm.generate(prompts, sps, use_tqdm=False)
        state = torch.get_rng_state()
        torch.manual_seed(5)
        b = llm.generate(prompts, sps, use_tqdm=False)
        assert [o["token_ids"] for o in a] == [o["token_ids"] for o in b]       # torch's loop on the global generator, as before
        assert torch.equal(state, torch.get_rng_state())
        assert llm.model_runner._ar_sampler is None
        llm.exit()


def test_generate_plants_one_seed_per_request_after_the_fold(monkeypatch):
    monkeypatch.setattr(LLMEngine, "generate", lambda self, prompts, sps, **kw: sps)
    llm = LLM.__new__(LLM)
    prompts = [[1], [2], [3]]
    sp = planted(0.8, 4, top_k=5, top_p=0.9, jacobi_lockstep=True)
    got = llm.generate(prompts, sp, seed=100)
    assert [g.seed for g in got] == [100, 101, 102] and len({id(g) for g in got}) == 3
    assert not hasattr(sp, "seed")                                         # the caller's object is not written to
    assert all((g.top_k, g.top_p, g.jacobi_lockstep, g.temperature) == (5, 0.9, True, 0.8) for g in got)
    got = llm.generate(prompts, [sp, planted(0.5, 4), sp], seed=[7, None, 9], jacobi_enabled=False)
    assert [getattr(g, "seed", None) for g in got] == [7, None, 9]
    with pytest.raises(ValueError):
        llm.generate(prompts, sp, seed=[1, 2])
    assert llm.generate(prompts, sp) is sp                                 # no seed: what the fold returns, as before
    # the fold's replace calls carry every planted attribute, a seed planted by the caller included
    sp2 = planted(0.8, 4, top_k=5, top_p=0.9, jacobi_lockstep=True, seed=3)
    for kw in (dict(greedy=True), dict(jacobi_block_len=8), dict(greedy=True, jacobi_enabled=True, jacobi_num_blocks=2)):
        f = llm.generate(prompts, sp2, **kw)
        assert f is not sp2 and (f.top_k, f.top_p, f.jacobi_lockstep, f.seed) == (5, 0.9, True, 3), kw
    assert llm.generate(prompts, sp2, greedy=True).temperature == 0.0
    assert llm.generate(prompts, sp2, jacobi_block_len=8).decode_strategy == "jacobi"


# ------------------------------------------------------------------------------------- 4. kernel vs oracle (GPU)
def to_dtype(x: np.ndarray, ldt: str) -> np.ndarray:
    return O.bf16_round(x) if ldt == "bf16" else x.astype(np.float32)


def expected_tokens(rows: np.ndarray, ldt: str, setting, which: np.ndarray, u: np.ndarray):
    """Row i samples distinct row which[i] at u[i] -> (oracle tokens, mask of the cases that may be left out: float32 rows whose
    u * total > 0 lies within 1e-9 * total of a CDF boundary)."""
    t, k, p = setting
    probs = O.target_probs(rows, t, ldt, k or None, p or None)
    cdfs = np.cumsum(probs.astype(np.float64), axis=1)
    want, near = np.zeros(len(u), dtype=np.int64), np.zeros(len(u), dtype=bool)
    for i, (d, ui) in enumerate(zip(which, u)):
        want[i] = O.inverse_cdf_sample(probs[d], float(ui))
        if ldt == "f32" and ui > 0:
            c, thr = cdfs[d], float(ui) * float(cdfs[d][-1])
            near[i] = np.abs(c - thr).min() <= 1e-9 * c[-1]
    return want, near


@functools.lru_cache(maxsize=None)
def kernel_case(V: int, R: int, ldt: str, setting, neg_inf: bool = False):
    """Inputs and expected tokens of one (shape, dtype, setting): min(R, 5) distinct rows, row i = distinct row i % 5, three
    passes of uniforms (random 24-bit ones, all 0.0, all the largest float32 below 1).  The last logit of a float32 row equals the
    row's largest, so that the largest uniform falls inside an interval of some width rather than among the boundaries of a
    tail of tiny probabilities (bf16 rows, whose sums are exact, keep their random tails).  The seed is the first one that leaves out at most 1 % of the cases."""
    D = min(R, 5)
    which = np.arange(R) % D
    for seed in range(20):
        rng = np.random.default_rng([V, R, int(setting[0] * 10), setting[1], int(setting[2] * 100), ldt == "bf16", neg_inf, seed])
        x = (rng.standard_normal((D, V)) * 2.5).astype(np.float32)
        if ldt == "f32":
            x[:, -1] = x[:, :-1].max(axis=1) if V > 1 else 0.0
        if neg_inf and V > 1:
            x[rng.random((D, V)) < 0.3] = -np.inf
            x[:, 0] = -np.inf                                             # u = 0 must skip it
            x[np.arange(D), rng.integers(1, V, D)] = 1.0                  # every row keeps some mass
            if V > 2:
                x[0, -1] = -np.inf                                        # the largest u must stop in front of it
                x[0, 1] = 1.0
        x = to_dtype(x, ldt)
        us = np.stack([(rng.integers(0, 1 << 24, R) * 2.0 ** -24).astype(np.float32), np.zeros(R, np.float32), np.full(R, U_MAX, np.float32)])
        want, near = zip(*(expected_tokens(x, ldt, setting, which, u) for u in us))
        want, near = np.stack(want), np.stack(near)
        if near.mean() <= 0.01:
            return x, which, us, want, near
    raise AssertionError("no seed leaves out at most 1 % of the cases")


def gpu_logits(x: np.ndarray, which: np.ndarray, ldt: str, pad: int = 0) -> torch.Tensor:
    """The R rows on the device in their dtype; pad > 0: a view with row_stride = V + pad into a buffer of NaNs."""
    t = torch.from_numpy(x[which]).to(torch.bfloat16 if ldt == "bf16" else torch.float32)
    if not pad:
        return t.to(DEV)
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)[:, :t.shape[1]]


def gpu_draw(smp: "ops.ARSampler", logits: torch.Tensor, setting, u: np.ndarray) -> np.ndarray:
    R = logits.shape[0]
    if R > smp.rows:
        smp._alloc(R)
    out = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    smp._draw(logits, setting, torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(DEV), out)
    return out.cpu().numpy()


def run_case(V, R, ldt, setting, pad=0, neg_inf=False):
    x, which, us, want, near = kernel_case(V, R, ldt, setting, neg_inf)
    assert near.mean() <= 0.01
    smp = ops.ARSampler(DEV, R)
    lg = gpu_logits(x, which, ldt, pad)
    assert lg.stride(0) == V + pad
    for u, w, nr in zip(us, want, near):
        got = gpu_draw(smp, lg, setting, u)
        assert ((got >= 0) & (got < V)).all()
        bad = np.flatnonzero((got != w) & ~nr)
        assert bad.size == 0, (bad[:5], got[bad[:5]], w[bad[:5]], u[bad[:5]])
        if neg_inf:
            assert np.isfinite(x[which, got]).all()                       # an id without mass is never drawn
    return want


SETTINGS = [(1.0, 0, 0.0), (0.8, 5, 0.0), (0.3, 0, 0.9), (0.8, 5, 0.9), (0.3, 5, 0.0), (1.0, 0, 0.9), (0.8, 0, 0.0), (0.3, 5, 0.9)]
SHAPES = [(V, R) for V in (1, 1000, 2048, 152064) for R in (1, 3, 65)]


@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"V{s[0]}-R{s[1]}")
def test_draws_match_the_oracle(shape, ldt):
    """Every shape in both dtypes; the temperature and the filters rotate over the shapes so that each of T in {1, 0.8, 0.3}
    and each of {none, top_k, top_p, both} meets small and large vocabularies, single rows and more rows than a wavefront."""
    V, R = shape
    i = SHAPES.index(shape) * 3 + (ldt == "f32")
    want = run_case(V, R, ldt, SETTINGS[i % len(SETTINGS)])
    if V > 1 and R > 1:
        assert len(np.unique(want)) > 1


@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
@pytest.mark.parametrize("setting", SETTINGS, ids=str)
def test_every_setting_at_a_vocabulary_that_is_no_multiple_of_a_vector(setting, ldt):
    run_case(1000, 3, ldt, setting)


@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
@pytest.mark.parametrize("V,pad", [(1000, 24), (1000, 3), (2048, 8), (152064, 64)])
def test_strided_rows(V, pad, ldt):
    """row_stride > V, with NaNs between the rows; pad = 3: rows that do not start on a 16-byte boundary."""
    run_case(V, 3, ldt, (0.8, 0, 0.0) if pad != 8 else (0.8, 5, 0.9), pad=pad)


@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
@pytest.mark.parametrize("setting", [(1.0, 0, 0.0), (0.8, 5, 0.9)], ids=str)
@pytest.mark.parametrize("V,R", [(2, 3), (1000, 65), (152064, 3)])
def test_ids_without_mass_are_never_drawn(V, R, setting, ldt):
    run_case(V, R, ldt, setting, neg_inf=True)


@GPU
@pytest.mark.parametrize("setting", [(0.8, 0, 0.0), (1.0, 20, 0.0), (0.3, 0, 0.9)], ids=str)
def test_the_floats_on_either_side_of_a_cdf_boundary_bf16(setting):
    """bf16 rows (exact sums): for boundaries c_i all along the CDF, the float32 nearest to c_i / total and its two neighbours.
    One float32 step moves u * total by >= 2^-25 * total, the sums are exact, so oracle and kernel must agree on every one, and
    the three tokens straddle the boundary."""
    V = 1000
    rng = np.random.default_rng(77)
    x = to_dtype((rng.standard_normal((1, V)) * 2.0).astype(np.float32), "bf16")
    p = O.target_probs(x, setting[0], "bf16", setting[1] or None, setting[2] or None)[0]
    c = np.cumsum(p.astype(np.float64))
    ids = np.flatnonzero(p > 0)[:-1]
    ids = ids[np.linspace(0, len(ids) - 1, min(len(ids), 200)).astype(int)]
    mid = (c[ids] / c[-1]).astype(np.float32)
    u = np.unique(np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1))]))
    u = u[(u >= 0) & (u < 1)]
    want = np.array([O.inverse_cdf_sample(p, float(v)) for v in u])
    assert len(np.unique(want)) >= len(ids)                               # both sides of the boundaries are there
    lg = torch.from_numpy(x).to(torch.bfloat16).to(DEV).expand(len(u), V).contiguous()
    got = gpu_draw(ops.ARSampler(DEV, len(u)), lg, setting, u)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]


@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
@pytest.mark.parametrize("setting", [(1.0, 0, 0.0), (0.8, 50, 0.9)], ids=str)
def test_stratified_uniforms_reproduce_the_distribution(setting, ldt):
    """u_i = (i + 0.5) / N over N = 4096 copies of one row: id v is drawn for the u in [c_(v-1), c_v) / total, N * p_v of them
    give or take one."""
    V, Ncopies = 1024, 4096
    rng = np.random.default_rng(5)
    x = to_dtype((rng.standard_normal((1, V)) * 2.0).astype(np.float32), ldt)
    p = O.target_probs(x, setting[0], ldt, setting[1] or None, setting[2] or None)[0].astype(np.float64)
    u = ((np.arange(Ncopies) + 0.5) / Ncopies).astype(np.float32)
    lg = torch.from_numpy(x).to(torch.bfloat16 if ldt == "bf16" else torch.float32).to(DEV).expand(Ncopies, V).contiguous()
    got = gpu_draw(ops.ARSampler(DEV, Ncopies), lg, setting, u)
    counts = np.bincount(got, minlength=V)
    assert counts.sum() == Ncopies and np.abs(counts - Ncopies * p / p.sum()).max() <= 1.0
    assert (counts[p == 0] == 0).all()


@GPU
def test_a_rows_token_does_not_depend_on_its_neighbours():
    """ARSampler on fixed logits: whole batch, reversed, shuffled, row by row, and with every row given the same setting as its
    neighbours — a row's token is a function of its logits, setting and uniform."""
    V, B = 1000, 12
    rng = np.random.default_rng(9)
    x = to_dtype((rng.standard_normal((B, V)) * 2.5).astype(np.float32), "bf16")
    kinds = [(0.8, 0, 0.0), (0.8, 5, 0.0), (0.0, 0, 0.0), (0.3, 0, 0.9), (1.0, 7, 0.8)]
    settings = [kinds[i % len(kinds)] for i in range(B)]
    u = (rng.integers(0, 1 << 24, B) * 2.0 ** -24).astype(np.float32)
    lg = torch.from_numpy(x).to(torch.bfloat16).to(DEV)
    smp = ops.ARSampler(DEV, 4)                                           # grows on demand
    base = smp.sample(lg, settings, u)
    assert base == [oracle_token(x[i], "bf16", settings[i], u[i]) for i in range(B)]
    for order in (list(range(B))[::-1], rng.permutation(B).tolist()):
        got = smp.sample(lg[order].contiguous(), [settings[i] for i in order], u[order])
        assert got == [base[i] for i in order]
    assert [smp.sample(lg[i:i + 1], [settings[i]], u[i:i + 1])[0] for i in range(B)] == base
    for s in set(settings):                                               # another grouping: the rows of one setting, as one batch
        idx = [i for i in range(B) if settings[i] == s]
        assert smp.sample(lg[idx].contiguous(), [s] * len(idx), u[idx]) == [base[i] for i in idx]
    one = smp.sample(lg, [kinds[1]] * B, u)                               # one setting: the logits are read where they are
    assert one == [oracle_token(x[i], "bf16", kinds[1], u[i]) for i in range(B)]


@GPU
def test_argument_validation():
    lib = N.lib()
    assert lib.jf_rs_draw_workspace_bytes(5) == lib.jf_rs_step_workspace_bytes(5) and lib.jf_rs_draw_workspace_bytes(0) == 0
    R, V = 2, 64
    lg = torch.zeros((R, V), dtype=torch.float32, device=DEV)
    f = torch.zeros((R,), dtype=torch.float32, device=DEV)
    tok = torch.zeros((R,), dtype=torch.int64, device=DEV)
    nb = int(lib.jf_rs_draw_workspace_bytes(R))
    ws = torch.zeros((nb // 8 + 2,), dtype=torch.float64, device=DEV)
    p, s = ops._ptr, ops._stream(torch.device(DEV))
    call = lambda **k: lib.jf_rs_draw_rows(*[k.get(n, d) for n, d in (("logits", p(lg)), ("dtype", N.JF_F32), ("R", R), ("V", V), ("stride", V),
                                                                      ("row_max", p(f)), ("row_sumexp", p(f)), ("t", 1.0), ("filt", None), ("u", p(f)),
                                                                      ("tokens", p(tok)), ("ws", p(ws)), ("ws_bytes", nb), ("stream", s))])
    assert call(R=0) == N.JF_OK and call(R=-3) == N.JF_OK
    for bad in (dict(logits=None), dict(row_max=None), dict(row_sumexp=None), dict(u=None), dict(tokens=None), dict(ws=None), dict(dtype=7),
                dict(V=0), dict(V=1 << 31), dict(ws_bytes=nb - 1), dict(ws=C.c_void_p(ws.data_ptr() + 8)), dict(R=1 << 28)):
        assert call(**bad) == N.JF_E_INVALID, bad
        assert b"jf_rs_draw_rows" in lib.jf_last_error()


# ------------------------------------------------------------------------------------- 5. through LLM.generate (GPU)
@GPU
def test_generate_with_seeds_matches_the_oracle_and_repeats(model_dir, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.delenv("JF_AR_SAMPLER", raising=False)
    calls = spy_on_sampler(monkeypatch)
    with use_backend("hip"):
        llm = LLM(model_dir, tokenizer_path="none", device=device_for("hip"), max_model_len=512, max_num_batched_tokens=512, max_num_seqs=8)
        n = 12
        kinds = [dict(temperature=0.8), dict(temperature=0.7, top_k=5), dict(temperature=0.0), dict(temperature=1.0, top_p=0.9),
                 dict(temperature=0.3, top_k=20, top_p=0.8), dict(temperature=0.9), dict(temperature=0.6, top_p=0.5)]
        sps = [planted(k.pop("temperature"), n, **k) for k in [dict(k) for k in kinds]]
        prompts = [[5 + i, 9, 200 - i, 31, 7][:3 + i % 3] for i in range(7)]
        seeds = [1000, 5, None, 77, 2 ** 40 + 3, 6, 123456789]
        V = 320
        key = lambda sp: (0.0, 0, 0.0) if sp.temperature == 0.0 else (float(sp.temperature),) + ops.active_filters(sp, V)
        out = llm.generate(prompts, sps, seed=seeds, use_tqdm=False)
        seen = check_calls(calls, {key(sp): sd for sp, sd in zip(sps, seeds)}, n)
        assert [o["token_ids"] for o in out] == [seen[key(sp)] for sp in sps]
        assert any(c[1] == "bf16" for c in calls)
        calls.clear()
        assert [o["token_ids"] for o in llm.generate(prompts, sps, seed=seeds, use_tqdm=False)] == [o["token_ids"] for o in out]
        calls.clear()
        alone = llm.generate(prompts[4:5], sps[4:5], seed=seeds[4:5], use_tqdm=False)      # its stream does not know the batch
        check_calls(calls, {key(sps[4]): seeds[4]}, n)
        assert len(alone[0]["token_ids"]) == n
        llm.exit()


@GPU
def test_generate_without_seed_never_builds_the_sampler(model_dir, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.delenv("JF_AR_SAMPLER", raising=False)
    calls = spy_on_sampler(monkeypatch)
    with use_backend("hip"):
        llm = LLM(model_dir, tokenizer_path="none", device=device_for("hip"), max_model_len=512, max_num_batched_tokens=512, max_num_seqs=4)
        torch.manual_seed(0)
        out = llm.generate([[1, 2, 3, 4], [9, 8, 7]], [planted(0.8, 8, top_k=5), planted(0.0, 8)], use_tqdm=False)
        assert [len(o["token_ids"]) for o in out] == [8, 8]
        assert llm.model_runner._ar_sampler is None and not calls
        llm.exit()
