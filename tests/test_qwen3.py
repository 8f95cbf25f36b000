"""Qwen3 checkpoints: config / loader rules, the QK-norm + RoPE + KV-append launch (``jf_qknorm_rope_kv_append``) against a float64
numpy reference of its definition, the forward against transformers' Qwen3ForCausalLM and the decoders end to end.

The definition under test (include/jacobiforcing.h): for every q and k head x[0..D) of every token, with w the q or the k norm weight,
y = x * rsqrt(mean x^2 + eps) * w and then the rotate-half RoPE of y, everything in float32, one rounding at the store; v heads are
copied bit for bit.

Comparison rule of the kernel tests: with a, b the two float64 products of a rotated element (want = a -+ b),
|got - want| <= 2^-18 (|a| + |b|) for f32 and <= 2^-7 |want| + 2^-18 (|a| + |b|) for bf16: one bf16 ulp on top of the float32
chain's error.  v heads and every cache element the call must not touch are compared as bits."""
import fnmatch
import ctypes as C
import json
import os
import re
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from jacobiforcing_amd import LLM, SamplingParams
from jacobiforcing_amd import _native as N
from jacobiforcing_amd import ops
from jacobiforcing_amd.modeling import qwen2
from jacobiforcing_amd.ops import qknorm_rope_kv_append
from jacobiforcing_amd.modeling.qwen2 import Qwen2Config, Qwen2Model, Qwen2Weights, StaticKVCache, load_model_directory

from .backends import device_for, use_backend

ROOT = Path(__file__).resolve().parents[1]
GPU = pytest.mark.gpu
DEV = "cuda:0"
SYMBOL = "jf_qknorm_rope_kv_append"
BACKENDS = [pytest.param("hostsim", id="hostsim"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]

# nq * head_dim = 128 != hidden_size = 64, tied embeddings
Q3 = dict(vocab_size=320, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
          head_dim=32, max_position_embeddings=1024, rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True,
          eos_token_id=319, pad_token_id=318, model_type="qwen3")
Q2 = dict(vocab_size=320, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
          max_position_embeddings=1024, rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=False, eos_token_id=319,
          pad_token_id=318, model_type="qwen2")


def hf_tensors(cfg: dict, seed=0, std=0.3):
    """A checkpoint of ``cfg`` under HF's tensor names (float32): what save_pretrained writes for Qwen2 / dense Qwen3."""
    g = torch.Generator().manual_seed(seed)
    H, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    nq, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or H // nq
    q3 = cfg.get("model_type") == "qwen3"
    rnd = lambda *s, sd=std: torch.randn(*s, generator=g) * sd
    t = {"model.embed_tokens.weight": rnd(V, H), "model.norm.weight": 1 + rnd(H, sd=0.1)}
    if not cfg.get("tie_word_embeddings"):
        t["lm_head.weight"] = rnd(V, H)
    for i in range(cfg["num_hidden_layers"]):
        pre = f"model.layers.{i}."
        t[pre + "input_layernorm.weight"] = 1 + rnd(H, sd=0.1)
        t[pre + "post_attention_layernorm.weight"] = 1 + rnd(H, sd=0.1)
        for n, rows in (("q", nq * hd), ("k", nkv * hd), ("v", nkv * hd)):
            t[pre + f"self_attn.{n}_proj.weight"] = rnd(rows, H)
            if not q3:
                t[pre + f"self_attn.{n}_proj.bias"] = rnd(rows, sd=0.01)
        if q3:
            t[pre + "self_attn.q_norm.weight"] = 1 + rnd(hd, sd=0.5)
            t[pre + "self_attn.k_norm.weight"] = 1 + rnd(hd, sd=0.5)
        t[pre + "self_attn.o_proj.weight"] = rnd(H, nq * hd)
        t[pre + "mlp.gate_proj.weight"] = rnd(I, H)
        t[pre + "mlp.up_proj.weight"] = rnd(I, H)
        t[pre + "mlp.down_proj.weight"] = rnd(H, I)
    return t


def write_dir(path: Path, cfg: dict, tensors: dict) -> str:
    from safetensors.torch import save_file
    path.mkdir(parents=True, exist_ok=True)
    (path / "config.json").write_text(json.dumps(cfg))
    save_file({k: v.contiguous() for k, v in tensors.items()}, str(path / "model.safetensors"))
    return str(path)


@pytest.fixture()
def qwen3_dir(tmp_path):
    return write_dir(tmp_path / "qwen3", Q3, hf_tensors(Q3))


# ------------------------------------------------------------------------------------- 1. boundary (CPU)
def test_the_entry_point_is_declared_exported_bound_and_counted():
    hdr = (ROOT / "include" / "jacobiforcing.h").read_text()
    assert re.search(r"^JF_API\s+int\s+" + SYMBOL + r"\s*\(", hdr, flags=re.M)
    emap = (ROOT / "jacobiforcing_amd" / "csrc" / "jf_exports.map").read_text()
    patterns = re.search(r"global:\s*([^;]+);", emap).group(1).split()
    assert any(fnmatch.fnmatchcase(SYMBOL, pat) for pat in patterns)
    import __graft_entry__ as G
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(G.build_hip())], text=True)
    assert SYMBOL in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert SYMBOL in N.EXPORTED_SYMBOLS and len(N._SIGNATURES[SYMBOL][1]) == 23
    assert N._SIGNATURES[SYMBOL][1][9] is C.c_float                                # eps travels as a float
    assert hasattr(ops, "qknorm_rope_kv_append")
    assert int(re.search(r"#define JF_VERSION (\d+)", hdr).group(1)) == 600          # an addition only
    n_hdr = len(re.findall(r"^JF_API\s", hdr, flags=re.M))
    assert n_hdr == len(N.EXPORTED_SYMBOLS)
    for doc in ("INTEGRATION.md", "COVERAGE.md"):
        assert f"{n_hdr} entry points" in (ROOT / doc).read_text(), doc


# ------------------------------------------------------------------------------------- 2. argument validation (CPU, the real library)
def test_argument_validation_needs_no_gpu():
    """Every JF_E_INVALID path and N == 0 return in front of the first launch: the real library, pointers that are never read."""
    lib = N.load()
    fake = C.c_void_p(1 << 20)                                            # 16-byte aligned, never dereferenced
    base = (("qkv", fake), ("dtype", N.JF_BF16), ("N", 6), ("T", 3), ("nq", 4), ("nkv", 2), ("D", 128), ("qn", fake), ("kn", fake),
            ("eps", 1e-6), ("positions", fake), ("cos", fake), ("sin", fake), ("q_out", fake), ("k_cache", fake), ("v_cache", fake),
            ("slot_main", fake), ("S_max", 64), ("k_cand", None), ("v_cand", None), ("slot_cand", None), ("T_max", 0), ("stream", None))
    call = lambda **k: getattr(lib, SYMBOL)(*[k.get(n, d) for n, d in base])
    assert call(N=0) == N.JF_OK and call(N=-2) == N.JF_OK and call(N=0, qkv=None, qn=None, eps=-1.0) == N.JF_OK
    bad_cases = [dict(qkv=None), dict(positions=None), dict(cos=None), dict(sin=None), dict(q_out=None), dict(k_cache=None),
                 dict(v_cache=None), dict(slot_main=None), dict(qn=None), dict(kn=None), dict(eps=-1e-6), dict(eps=float("nan")),
                 dict(eps=float("-inf")), dict(dtype=7), dict(T=0), dict(N=7), dict(nq=0), dict(nkv=0), dict(nq=3), dict(D=0),
                 dict(D=127), dict(S_max=0), dict(slot_cand=fake), dict(slot_cand=fake, k_cand=fake, v_cand=fake, T_max=0),
                 dict(slot_cand=fake, k_cand=fake, T_max=8)]
    for bad in bad_cases:
        assert call(**bad) == N.JF_E_INVALID, bad
        assert SYMBOL.encode() in lib.jf_last_error(), bad


# ------------------------------------------------------------------------------------- 3. config (CPU)
def test_config_families(tmp_path):
    (tmp_path / "q3.json").write_text(json.dumps(Q3))
    c3 = Qwen2Config.from_json(tmp_path / "q3.json")
    assert c3.qk_norm is True and c3.attention_bias is False and c3.head_dim == 32 and c3.tie_word_embeddings is True
    assert c3.num_attention_heads * c3.head_dim == 128 != c3.hidden_size
    (tmp_path / "q2.json").write_text(json.dumps(Q2))
    c2 = Qwen2Config.from_json(tmp_path / "q2.json")
    assert c2 == Qwen2Config(vocab_size=320, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                             num_key_value_heads=2, head_dim=16, rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=1024,
                             tie_word_embeddings=False, eos_token_id=319, pad_token_id=318)
    assert c2.qk_norm is False and c2.attention_bias is True
    assert Qwen2Config().qk_norm is False and Qwen2Config().attention_bias is True and Qwen2Config.tiny().qk_norm is False
    no_type = {k: v for k, v in Q2.items() if k != "model_type"}                  # the toy checkpoint's kind of config keeps loading
    (tmp_path / "nt.json").write_text(json.dumps(no_type))
    assert Qwen2Config.from_json(tmp_path / "nt.json") == c2
    # an explicit attention_bias wins over the family default; a harmless rope / layer description is accepted
    ok = dict(Q3, attention_bias=True, layer_types=["full_attention"] * 2, use_sliding_window=False, rope_scaling=None,
              rope_parameters={"rope_type": "default", "rope_theta": 5e5})
    ok.pop("rope_theta")
    (tmp_path / "ok.json").write_text(json.dumps(ok))
    c = Qwen2Config.from_json(tmp_path / "ok.json")
    assert c.qk_norm and c.attention_bias and c.rope_theta == 5e5


@pytest.mark.parametrize("extra, field", [
    (dict(model_type="qwen3_moe"), "model_type"), (dict(num_experts=8), "num_experts"),
    (dict(layer_types=["full_attention", "sliding_attention"]), "layer_types"), (dict(use_sliding_window=True), "use_sliding_window"),
    (dict(rope_scaling={"rope_type": "yarn", "factor": 4.0}), "rope_scaling"),
    (dict(rope_parameters={"rope_type": "linear", "factor": 2.0, "rope_theta": 1e6}), "rope_parameters")],
    ids=["moe", "experts", "layer_types", "sliding_window", "rope_scaling", "rope_parameters"])
def test_config_refusals_name_their_field(tmp_path, extra, field):
    (tmp_path / "config.json").write_text(json.dumps(dict(Q3, **extra)))
    with pytest.raises(ValueError, match=field):
        Qwen2Config.from_json(tmp_path / "config.json")


# ------------------------------------------------------------------------------------- 4. loaders (CPU)
def test_loaders_are_strict_in_both_directions(tmp_path):
    t3, t2 = hf_tensors(Q3), hf_tensors(Q2)
    cfg, w = load_model_directory(write_dir(tmp_path / "good3", Q3, t3), "cpu")
    assert cfg.qk_norm and all(L["bqkv"] is None and L["qn"].shape == (32,) and L["kn"].shape == (32,) for L in w.layers)
    assert torch.equal(w.layers[1]["kn"], t3["model.layers.1.self_attn.k_norm.weight"]) and w.lm_head is w.embed
    assert w.layers[0]["wqkv"].shape == (8 * 32, 64) and w.layers[0]["wo"].shape == (64, 128)
    cfg, w = load_model_directory(write_dir(tmp_path / "good2", Q2, t2), "cpu")
    assert all(L["bqkv"].shape == (8 * 16,) and "qn" not in L and "kn" not in L for L in w.layers)
    # a tensor the config calls for is missing
    name = "model.layers.1.self_attn.k_norm.weight"
    with pytest.raises(KeyError, match=re.escape(name)):
        load_model_directory(write_dir(tmp_path / "a", Q3, {k: v for k, v in t3.items() if k != name}), "cpu")
    name = "model.layers.0.self_attn.v_proj.bias"
    with pytest.raises(KeyError, match=re.escape(name)):
        load_model_directory(write_dir(tmp_path / "b", Q2, {k: v for k, v in t2.items() if k != name}), "cpu")
    # a tensor the config does not call for is present
    name = "model.layers.1.self_attn.q_norm.weight"
    with pytest.raises(ValueError, match=re.escape(name)):
        load_model_directory(write_dir(tmp_path / "c", Q2, dict(t2, **{name: torch.ones(16)})), "cpu")
    name = "model.layers.0.self_attn.k_proj.bias"
    with pytest.raises(ValueError, match=re.escape(name)):
        load_model_directory(write_dir(tmp_path / "d", Q3, dict(t3, **{name: torch.zeros(64)})), "cpu")
    # the same rules through load_state_dict
    c3 = Qwen2Config.from_json(tmp_path / "good3" / "config.json")
    w3 = Qwen2Weights(c3, "cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match=re.escape(name)):
        w3.load_state_dict(dict(t3, **{name: torch.zeros(64)}), c3)
    with pytest.raises(KeyError, match="q_norm"):
        w3.load_state_dict({k: v for k, v in t3.items() if "layers.0.self_attn.q_norm" not in k}, c3)


def test_random_init_weights_per_family():
    c2 = Qwen2Config.tiny()
    w2 = Qwen2Weights(c2, "cpu", dtype=torch.float32, seed=5)
    assert all("qn" not in L and "kn" not in L and L["bqkv"].shape == ((4 + 2 * 2) * 32,) for L in w2.layers)
    c3 = Qwen2Config(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                     num_key_value_heads=2, head_dim=32, qk_norm=True, attention_bias=False, tie_word_embeddings=True)
    w3 = Qwen2Weights(c3, "cpu", dtype=torch.float32, seed=5)
    for L in w3.layers:
        assert L["bqkv"] is None and torch.equal(L["qn"], torch.ones(32)) and torch.equal(L["kn"], torch.ones(32))
        assert L["wqkv"].shape == (8 * 32, 64) and L["wo"].shape == (64, 4 * 32)
    assert w3.lm_head is w3.embed


# ------------------------------------------------------------------------------------- 5. the forward against transformers (CPU)
def _hf_qwen3(tr, tie, vocab=97, init=0.02, seed=0):
    hf_cfg = tr.Qwen3Config(vocab_size=vocab, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                            num_key_value_heads=2, head_dim=32, max_position_embeddings=1024, rms_norm_eps=1e-6,
                            tie_word_embeddings=tie, attention_dropout=0.0, use_sliding_window=False, attention_bias=False,
                            initializer_range=init, eos_token_id=vocab - 1, pad_token_id=vocab - 2)
    torch.manual_seed(seed)
    hf = tr.Qwen3ForCausalLM(hf_cfg).eval().float()
    with torch.no_grad():
        for layer in hf.model.layers:                                  # ones by default: randomised so that they are exercised
            for nrm in (layer.self_attn.q_norm, layer.self_attn.k_norm):
                nrm.weight.copy_(1 + 0.5 * torch.randn(32))
    return hf


@pytest.mark.parametrize("tie", [True, False], ids=["tied", "untied"])
def test_forward_matches_hf_qwen3(tie):
    """Logits against transformers' Qwen3ForCausalLM on the tiny config (CPU, fp32): a prefix of 9 tokens, then 14 on the cache."""
    tr = pytest.importorskip("transformers")
    with use_backend("hostsim"):
        hf = _hf_qwen3(tr, tie)
        model = Qwen2Model.from_hf(hf)
        cfg = model.cfg
        assert cfg.qk_norm and not cfg.attention_bias and cfg.head_dim == 32 and cfg.tie_word_embeddings == tie
        assert (model.w.lm_head is model.w.embed) == tie
        ids = torch.randint(0, 97, (1, 23))
        with torch.no_grad():
            ref = hf(input_ids=ids).logits[0]
        cache = StaticKVCache(cfg, 1, 64, 0, 1, "cpu", dtype=torch.float32)
        z = torch.zeros(1, dtype=torch.int32)
        l1 = model.forward(ids[:, :9], torch.arange(9, dtype=torch.int32).view(1, 9), cache, z, z - 1, z + 9, z, False)
        l2 = model.forward(ids[:, 9:], torch.arange(9, 23, dtype=torch.int32).view(1, 14), cache, z, z - 1, z + 14, z + 9, False)
        got = torch.cat([l1, l2], 0)
        assert torch.allclose(got, ref, atol=2e-4, rtol=2e-4), float((got - ref).abs().max())


# ------------------------------------------------------------------------------------- 6. / 11. end to end
def _greedy(n, **kw):
    return SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True, **kw)


PROMPTS = [[5, 9, 200, 31, 7], [100, 101, 102, 103, 104, 105, 106, 107, 108], [250, 3]]


@pytest.mark.parametrize("backend", BACKENDS)
def test_llm_on_a_qwen3_directory_jacobi_matches_autoregressive(qwen3_dir, backend, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.setenv("JF_DTYPE", "float32")     # bf16 GEMV-vs-GEMM rounding flips near-tie argmaxes of a random model
    with use_backend(backend):
        llm = LLM(qwen3_dir, tokenizer_path="none", device=device_for(backend), max_model_len=512, max_num_batched_tokens=512,
                  max_num_seqs=4)
        cfg = llm.model_runner.model.cfg
        assert cfg.qk_norm and not cfg.attention_bias and llm.model_runner.weights.layers[0]["bqkv"] is None
        n = 32
        ar = llm.generate(PROMPTS, _greedy(n), use_tqdm=False)
        jac = llm.generate(PROMPTS, _greedy(n, decode_strategy="jacobi", jacobi_block_len=8), use_tqdm=False)
        mb = llm.generate(PROMPTS, _greedy(n, decode_strategy="jacobi_multiblock_rejection_recycling", jacobi_block_len=8,
                                           jacobi_max_blocks=2, jacobi_spawn_ratio=0.5), use_tqdm=False)
        assert [len(o["token_ids"]) for o in ar] == [n] * 3
        for a, j, m in zip(ar, jac, mb):
            assert j["token_ids"][:n] == a["token_ids"] and m["token_ids"][:n] == a["token_ids"]
        llm.exit()


@pytest.mark.parametrize("backend", BACKENDS)
def test_llm_on_a_qwen3_directory_paged_layout(qwen3_dir, backend, monkeypatch):
    monkeypatch.setenv("JF_INIT_STD", "0.3")
    monkeypatch.setenv("JF_DTYPE", "float32")
    with use_backend(backend):
        llm = LLM(qwen3_dir, tokenizer_path="none", device=device_for(backend), max_model_len=512, max_num_batched_tokens=512,
                  max_num_seqs=4, kv_cache_layout="paged")
        assert llm.model_runner.paged and llm.model_runner.model.cfg.qk_norm
        n = 24
        ar = llm.generate(PROMPTS, _greedy(n), use_tqdm=False)
        jac = llm.generate(PROMPTS, _greedy(n, decode_strategy="jacobi", jacobi_block_len=8), use_tqdm=False)
        for a, j in zip(ar, jac):
            assert len(a["token_ids"]) == n and j["token_ids"][:n] == a["token_ids"]
        llm.exit()


def test_hf_seam_driver_on_a_loaded_qwen3():
    """drivers.sb_math500.decode_one over hf_seam.jacobi_forward_greedy on Qwen2Model.from_hf of a Qwen3ForCausalLM decodes what
    drivers.ar_baseline.generate_greedy decodes token by token."""
    tr = pytest.importorskip("transformers")
    import random
    from jacobiforcing_amd import hf_seam
    from jacobiforcing_amd.drivers import ar_baseline, sb_math500
    with use_backend("hostsim"):
        model = Qwen2Model.from_hf(_hf_qwen3(tr, True, vocab=320, init=0.3, seed=2))
        assert model.cfg.qk_norm and model.w.layers[0]["bqkv"] is None
        me = types.SimpleNamespace(jf_backend=hf_seam.Qwen2Backend(model, max_seq_len=256, max_rows=1, max_tokens=64))
        row, toks = sb_math500.decode_one(me, PROMPTS[1], n=8, eos_id=None, alt_eos_id=None, max_new_tokens=40, max_calls=64,
                                          rng=random.Random(0))
        ar, _ = ar_baseline.generate_greedy(model, PROMPTS[1], max_new_tokens=len(toks))
        assert len(toks) >= 40 and toks == ar


# ------------------------------------------------------------------------------------- 7. routing
class _NoQknormSymbol:
    """A library whose new entry point is booby-trapped: looking it up fails the test."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        if name == SYMBOL:
            raise AssertionError(f"a model without q/k norms looked up {name}")
        return getattr(self._inner, name)


def _two_forwards(model, dev):
    """A prefill of 3 rows and a second forward with candidate rows on top of it (main + candidate caches written)."""
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(4)
    P, T1, T2 = 3, 6, 5
    lens = [6, 4, 5]
    cache = StaticKVCache(model.cfg, P, 48, 2, 8, dev, dtype=model.dtype)
    ids1 = torch.randint(0, model.cfg.vocab_size, (P, T1), generator=g).to(dev)
    pos1 = torch.arange(T1, dtype=torch.int32, device=dev).view(1, T1).expand(P, T1).contiguous()
    l1 = model.forward(ids1, pos1, cache, row_prompt=i32([0, 1, 2]), row_cand=i32([-1] * P), row_len=i32(lens), kv_len_rows=i32([0] * P),
                       any_candidates=False, s_cur=T1)
    kv = i32(lens + [lens[0], lens[2]])
    ids2 = torch.randint(0, model.cfg.vocab_size, (5, T2), generator=g).to(dev)
    pos2 = (kv.view(5, 1) + torch.arange(T2, dtype=torch.int32, device=dev).view(1, T2)).contiguous()
    l2 = model.forward(ids2, pos2, cache, row_prompt=i32([0, 1, 2, 0, 2]), row_cand=i32([-1, -1, -1, 0, 5]), row_len=i32([5, 3, 5, 4, 5]),
                       kv_len_rows=kv, any_candidates=True, s_cur=max(lens) + T2, n_main=3)
    return (l1, l2), cache


def test_a_qwen2_model_never_looks_the_new_symbol_up(monkeypatch):
    monkeypatch.setattr(qwen2, "QKNORM_FUSED", True)
    with use_backend("hostsim") as lib:
        N._LIB = _NoQknormSymbol(lib)                                # use_backend puts the previous library back on exit
        with pytest.raises(AssertionError):
            getattr(N.lib(), SYMBOL)
        cfg = Qwen2Config.tiny()
        model = Qwen2Model(cfg, Qwen2Weights(cfg, torch.device("cpu"), dtype=torch.float32, seed=1))
        logits, cache = _two_forwards(model, "cpu")
        assert all(torch.isfinite(l).all() for l in logits) and cache.ck[0].any()
        # and neither does a Qwen3 model off the GPU: the torch normalisation in front of the unchanged launch
        c3 = Qwen2Config.tiny()
        c3.qk_norm, c3.attention_bias = True, False
        m3 = Qwen2Model(c3, Qwen2Weights(c3, torch.device("cpu"), dtype=torch.float32, seed=1))
        logits, cache = _two_forwards(m3, "cpu")
        assert all(torch.isfinite(l).all() for l in logits) and cache.ck[0].any()


# ------------------------------------------------------------------------------------- 8. the float64 reference
def reference(x, qn, kn, eps, pos, cos, sin, nq, nkv):
    """x [N, heads, D], qn / kn [D], cos / sin [n_pos, D/2] (all float64 images of the kernel's inputs), pos [N] ->
    (out [N, heads, D], mag [N, heads, D]): out is the definition in float64 (v heads = x), mag = |a| + |b| of the two products of
    every rotated element (0 on v heads)."""
    x = np.asarray(x, dtype=np.float64)
    Ntok, heads, D = x.shape
    half = D // 2
    w = np.concatenate([np.broadcast_to(qn, (nq, D)), np.broadcast_to(kn, (nkv, D))]).astype(np.float64)[None]
    xr = x[:, :nq + nkv]
    y = xr / np.sqrt((xr * xr).mean(-1, keepdims=True) + np.float64(eps)) * w
    c, s = cos[pos][:, None, :].astype(np.float64), sin[pos][:, None, :].astype(np.float64)
    y1, y2 = y[..., :half], y[..., half:]
    out, mag = x.copy(), np.zeros_like(x)
    out[:, :nq + nkv] = np.concatenate([y1 * c - y2 * s, y2 * c + y1 * s], -1)
    mag[:, :nq + nkv] = np.concatenate([np.abs(y1 * c) + np.abs(y2 * s), np.abs(y2 * c) + np.abs(y1 * s)], -1)
    return out, mag


def test_reference_agrees_with_hf_in_float64():
    pytest.importorskip("transformers")
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm, apply_rotary_pos_emb
    g = torch.Generator().manual_seed(3)
    Ntok, nq, nkv, D, eps = 5, 3, 1, 32, 1e-6
    x = torch.randn(Ntok, nq + 2 * nkv, D, generator=g, dtype=torch.float64)
    x[2, 1] = 0.0
    x[3, 0] *= 3e3
    qn, kn = (1 + 0.5 * torch.randn(D, generator=g, dtype=torch.float64) for _ in range(2))
    pos = torch.tensor([7, 0, 4095, 13, 2])
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    fr = torch.outer(torch.arange(4096, dtype=torch.float64), inv)
    x[4, 2] *= 1e-3                                                     # mean x^2 ~ eps: where eps sits in the formula shows
    got, mag = reference(x.numpy(), qn.numpy(), kn.numpy(), eps, pos.numpy(), fr.cos().numpy(), fr.sin().numpy(), nq, nkv)
    emb = torch.cat([fr, fr], -1)[pos]                                  # [N, D], HF's cos / sin layout

    def hf(norm_q, norm_k):
        with torch.no_grad():
            q = norm_q(x[:, :nq]).transpose(0, 1)[None]                 # [1, heads, N, D]
            k = norm_k(x[:, nq:nq + nkv]).transpose(0, 1)[None]
            qr, kr = apply_rotary_pos_emb(q, k, emb.cos()[None], emb.sin()[None])
        return torch.cat([qr[0].transpose(0, 1), kr[0].transpose(0, 1), x[:, nq + nkv:]], 1).numpy()

    # Qwen3RMSNorm.forward computes in float32 whatever it is given, so the class itself is compared at float32 accuracy and its
    # forward, restated line by line without the cast, at float64 accuracy; apply_rotary_pos_emb runs in float64 both times
    mods = []
    for w in (qn, kn):
        m = Qwen3RMSNorm(D, eps=eps).double()
        with torch.no_grad():
            m.weight.copy_(w)
        mods.append(m)
    assert np.allclose(got, hf(*mods), rtol=2e-6, atol=1e-6)
    f64 = lambda w: (lambda h: w * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)))
    want = hf(f64(qn), f64(kn))
    assert np.allclose(got, want, rtol=1e-12, atol=1e-13)
    assert np.array_equal(got[2, 1], np.zeros(D)) and np.array_equal(got[:, nq + nkv:], x[:, nq + nkv:].numpy())
    assert (mag[:, :nq + nkv] + 1e-300 >= np.abs(got[:, :nq + nkv])).all() and not mag[:, nq + nkv:].any()


# ------------------------------------------------------------------------------------- 9. the kernel (GPU)
_TABLES = {}


def _tables(D):
    """fp32 cos / sin [4096, D/2]: computed once per D and shared, never written."""
    if D not in _TABLES:
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
        fr = torch.outer(torch.arange(4096, dtype=torch.float32), inv)
        _TABLES[D] = (fr.cos().contiguous(), fr.sin().contiguous())
    return _TABLES[D]


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def kernel_case(ldt, D, nq, nkv, R, T, cand, misalign=0):
    """One call against the float64 reference.  Special heads: an all-zero one, one scaled by 3e3, one by 1e-3; every (token,
    head) carries its own magnitude on top of random values, so a row stored in another row's place cannot pass."""
    dtype = torch.bfloat16 if ldt == "bf16" else torch.float32
    Ntok, heads, G = R * T, nq + 2 * nkv, nq // nkv
    S_max, T_max, rows, crow = 16, 8, 4, 3
    g = torch.Generator().manual_seed(1000 * D + 100 * nq + 10 * R + T)
    x = torch.randn(Ntok, heads, D, generator=g) * (1 + 0.25 * torch.arange(Ntok * heads).view(Ntok, heads, 1))
    x[0, 1] = 0.0                                                       # a q head of zeros
    x[Ntok - 1, nq] *= 3e3                                              # a k head
    x[Ntok // 2, 0] *= 1e-3                                             # a q head
    x = x.to(dtype)
    buf = torch.zeros(Ntok * heads * D + 16, dtype=dtype)
    off = misalign // buf.element_size()
    buf[off:off + x.numel()] = x.view(-1)
    buf = buf.to(DEV)
    qkv = buf[off:off + x.numel()].view(Ntok, heads * D)
    assert qkv.is_contiguous() and qkv.data_ptr() % 16 == misalign
    qn, kn = ((1 + 0.5 * torch.randn(D, generator=g)).to(dtype) for _ in range(2))
    eps = 1e-6
    pos = torch.randint(0, 4096, (Ntok,), generator=g, dtype=torch.int32)       # not monotonic
    pos[0] = 4095
    cos, sin = _tables(D)
    perm = torch.randperm(rows * S_max, generator=g)[:Ntok]
    slot_main = perm.to(torch.int64)
    slot_cand = torch.randperm(crow * T_max, generator=g)[:Ntok].to(torch.int64)
    if Ntok > 1:
        slot_main[1::4] = -1
        slot_cand[::3] = -1
    else:
        slot_cand[0] = -1
    fill = 0x7F7F if dtype == torch.bfloat16 else 0x7F7F7F7F             # sentinel bits in every cache element
    ibits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    mk = lambda *s: torch.full(s, fill, dtype=ibits).view(dtype).to(DEV)
    kc, vc = mk(rows, nkv, S_max, D), mk(rows, nkv, S_max, D)
    ck, cv = mk(crow, nkv, T_max, D), mk(crow, nkv, T_max, D)
    args = (kc, vc, slot_main.to(DEV)) + ((ck, cv, slot_cand.to(DEV)) if cand else ())
    q = qknorm_rope_kv_append(qkv, T, nq, nkv, D, qn.to(DEV), kn.to(DEV), eps, pos.to(DEV), cos.to(DEV), sin.to(DEV), *args)
    torch.cuda.synchronize()

    f64 = lambda t: t.detach().cpu().float().numpy().astype(np.float64)
    want, mag = reference(f64(x), f64(qn), f64(kn), eps, pos.long().numpy(), f64(cos), f64(sin), nq, nkv)
    worst = [0.0]

    def close(got, w, m, what):
        bound = 2.0 ** -18 * m + (2.0 ** -7 * np.abs(w) if ldt == "bf16" else 0.0)
        err = np.abs(got - w)
        ok = err <= bound
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[0] = max(worst[0], float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))))
        assert ok.all(), (what, ldt, D, nq, nkv, R, T, int((~ok).sum()), float(err.max()))

    # q_out [R, nkv, G*T, D]: query row g*T + t of KV head kvh is head kvh*G + g of token r*T + t
    perm_q = lambda a: a[:, :nq].reshape(R, T, nkv, G, D).transpose(0, 2, 3, 1, 4).reshape(R, nkv, G * T, D)
    assert tuple(q.shape) == (R, nkv, G * T, D)
    close(f64(q), perm_q(want), perm_q(mag), "q_out")
    xb = _bits(x)
    for name, cache, vcache, slots, cap, on in (("main", kc, vc, slot_main, S_max, True), ("cand", ck, cv, slot_cand, T_max, cand)):
        kg, kb, vb = f64(cache), _bits(cache), _bits(vcache)
        touched = np.zeros(kb.shape[:3], dtype=bool)
        for i in range(Ntok if on else 0):
            s_ = int(slots[i])
            if s_ < 0:
                continue
            brow, p_ = divmod(s_, cap)
            touched[brow, :, p_] = True
            close(kg[brow, :, p_], want[i, nq:nq + nkv], mag[i, nq:nq + nkv], f"k {name}")
            assert np.array_equal(vb[brow, :, p_], xb[i, nq + nkv:]), f"v {name}: not a bit copy"
        sent = np.array(fill, dtype=np.int64).astype(kb.dtype)
        assert (kb[~touched] == sent).all() and (vb[~touched] == sent).all(), f"{name}: an element outside the slots was written"
        assert on or not touched.any()
    zero = f64(q)[0, 1 // G, (1 % G) * T + 0]
    assert not zero.any(), "the all-zero head"
    print(f"qknorm_rope {ldt} D={D} nq={nq} nkv={nkv} R={R} T={T} cand={cand} misalign={misalign}: worst error / bound = {worst[0]:.3f}")
    return worst[0]


@GPU
@pytest.mark.parametrize("cand", [True, False], ids=["cand", "nocand"])
@pytest.mark.parametrize("R, T", [(3, 5), (1, 1)], ids=["3x5", "1x1"])
@pytest.mark.parametrize("nq, nkv", [(4, 2), (3, 1)], ids=["4q2kv", "3q1kv"])
@pytest.mark.parametrize("D", [128, 64, 32, 96])
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
def test_kernel_matches_the_float64_reference(ldt, D, nq, nkv, R, T, cand):
    kernel_case(ldt, D, nq, nkv, R, T, cand)


@GPU
@pytest.mark.parametrize("ldt", ["bf16", "f32"])
def test_kernel_on_a_view_misaligned_by_8_bytes(ldt):
    kernel_case(ldt, 128, 4, 2, 3, 5, True, misalign=8)


@GPU
def test_kernel_general_path_forced_in_a_child_process():
    code = ("from tests.test_qwen3 import kernel_case\n"
            "for ldt in ('bf16', 'f32'):\n"
            "    for D in (128, 32):\n"
            "        kernel_case(ldt, D, 3, 1, 3, 5, True)\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, JF_ROPE_SCALAR="1"), capture_output=True, text=True,
                       timeout=300, cwd=str(ROOT))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1500:], r.stderr[-2000:])


@GPU
def test_binding_checks_the_weights():
    D = 32
    qkv = torch.zeros(2, 8 * D, device=DEV)
    pos = torch.zeros(2, dtype=torch.int32, device=DEV)
    cos, sin = (t.to(DEV) for t in _tables(D))
    kc = torch.zeros(1, 2, 4, D, device=DEV)
    sl = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    w = torch.ones(D, device=DEV)
    for qn, kn in ((w[:16], w), (w, w.to(torch.bfloat16)), (w, torch.ones(D)), (torch.ones(2 * D, device=DEV)[::2], w)):
        with pytest.raises(ValueError, match="norm weights"):
            ops.qknorm_rope_kv_append(qkv, 1, 4, 2, D, qn, kn, 1e-6, pos, cos, sin, kc, kc.clone(), sl)
    with pytest.raises(ValueError, match=SYMBOL):
        ops.qknorm_rope_kv_append(qkv, 1, 4, 2, D, w, w, -1.0, pos, cos, sin, kc, kc.clone(), sl)


# ------------------------------------------------------------------------------------- 10. the forward on the GPU
@GPU
def test_gpu_forward_fused_vs_torch_normalisation(monkeypatch):
    """fp32 weights, tiny Qwen3 (D = 32): logits with QKNORM_FUSED on and off agree at 2e-4; switched on, a forward calls the new
    entry once per layer and jf_rope_kv_append never; switched off, the other way round."""
    cfg = Qwen2Config.from_dict(Q3)
    w = Qwen2Weights(cfg, torch.device(DEV), dtype=torch.float32, seed=2, init_std=0.3)
    g = torch.Generator().manual_seed(9)
    for L in w.layers:
        L["qn"] = (1 + 0.5 * torch.randn(cfg.head_dim, generator=g)).to(DEV)
        L["kn"] = (1 + 0.5 * torch.randn(cfg.head_dim, generator=g)).to(DEV)
    model = Qwen2Model(cfg, w)
    calls = {"fused": 0, "plain": 0}
    fused, plain = ops.qknorm_rope_kv_append, ops.rope_kv_append
    monkeypatch.setattr(ops, "qknorm_rope_kv_append", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), fused(*a, **k))[1])
    monkeypatch.setattr(ops, "rope_kv_append", lambda *a, **k: (calls.__setitem__("plain", calls["plain"] + 1), plain(*a, **k))[1])
    monkeypatch.setattr(qwen2, "QKNORM_FUSED", True)
    la, ca = _two_forwards(model, DEV)
    assert calls == {"fused": 2 * cfg.num_hidden_layers, "plain": 0}, calls
    monkeypatch.setattr(qwen2, "QKNORM_FUSED", False)
    lb, cb = _two_forwards(model, DEV)
    assert calls == {"fused": 2 * cfg.num_hidden_layers, "plain": 2 * cfg.num_hidden_layers}, calls
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.isfinite(x).all() and float(x.abs().max()) > 0.1
        assert torch.allclose(x, y, atol=2e-4, rtol=2e-4), (i, float((x - y).abs().max()))
    for name in ("k", "v", "ck", "cv"):
        for li, (x, y) in enumerate(zip(getattr(ca, name), getattr(cb, name))):
            assert torch.allclose(x, y, atol=2e-4, rtol=2e-4), (name, li)
    assert ca.ck[0].any() and ca.k[0].any()                              # both caches were written
