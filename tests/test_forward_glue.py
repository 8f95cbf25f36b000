"""The forward's HIP glue (jf_attn_out_relayout, jf_forward_plan) against the torch code it replaces on the GPU.  Both are data
movement and integer arithmetic, so every comparison is bit for bit: no tolerance anywhere in this file."""
import pytest
import torch

from jacobiforcing_amd import _native as N
from jacobiforcing_amd import ops
from jacobiforcing_amd.modeling import qwen2
from jacobiforcing_amd.modeling.qwen2 import Qwen2Config, Qwen2Model, Qwen2Weights, StaticKVCache

from .backends import use_backend

GPU = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float32, id="f32")]
INT_OF = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def random_bits(shape, dtype, seed):
    """Every bit pattern is fair game for a copy: random words with NaNs, infinities and -0 planted."""
    g = torch.Generator().manual_seed(seed)
    it = INT_OF[dtype]
    lo, hi = (-2**15, 2**15) if it == torch.int16 else (-2**31, 2**31)
    x = torch.randint(lo, hi, shape, generator=g, dtype=torch.int64).to(it).reshape(-1)
    special = [0x7FC1, -0x8000, 0x7F80, -0x0080] if it == torch.int16 else [0x7FC00001, -0x80000000, 0x7F800000, -0x00800000]
    for i, s in enumerate(special):
        x[i::max(len(special), x.numel() // 7 or 1)] = s
    return x.reshape(shape).view(dtype)


# ------------------------------------------------------------------------------------- 1. relayout
def run_relayout(shape, dtype, transposed):
    """``transposed``: the input is the view of a [Rn, G*T, nkv, D] tensor the fused attention returns, else contiguous."""
    Rn, T, nkv, G, D = shape
    r0, it = 2, INT_OF[dtype]
    if transposed:
        oa = random_bits((Rn, G * T, nkv, D), dtype, seed=sum(shape)).to(DEV).transpose(1, 2)
    else:
        oa = random_bits((Rn, nkv, G * T, D), dtype, seed=sum(shape)).to(DEV)
    rows = (r0 + Rn + 1) * T
    sentinel = 0x5A5A
    out = torch.full((rows, nkv * G * D), sentinel, dtype=it, device=DEV).view(dtype)
    want = torch.full((rows, nkv * G * D), sentinel, dtype=it, device=DEV)
    want[r0 * T:(r0 + Rn) * T].view(Rn, T, nkv, G, D).copy_(oa.view(it).view(Rn, nkv, G, T, D).permute(0, 3, 1, 2, 4))
    ops.attn_out_relayout(oa, T, G, out[r0 * T:(r0 + Rn) * T])
    assert torch.equal(out.view(it), want)                       # the rows outside [r0*T, (r0+Rn)*T) keep the sentinel


@GPU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("transposed", [False, True], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 8), (3, 5, 2, 7, 128), (2, 33, 4, 7, 128), (5, 8, 2, 2, 32)], ids=str)
def test_relayout_matches_the_torch_expression(shape, transposed, dtype):
    run_relayout(shape, dtype, transposed)


@GPU
def test_relayout_head_dim_12_f32_passes_bf16_is_refused():
    """D = 12: three 16-byte vectors per head in f32; in bf16 a head is 24 bytes, no whole number of vectors: JF_E_INVALID from
    the library's argument check, in front of any launch."""
    run_relayout((2, 3, 2, 2, 12), torch.float32, False)
    run_relayout((2, 3, 2, 2, 12), torch.float32, True)
    oa = torch.zeros((2, 2, 2 * 3, 12), dtype=torch.bfloat16, device=DEV)
    out = torch.zeros((2 * 3, 2 * 2 * 12), dtype=torch.bfloat16, device=DEV)
    rc = N.lib().jf_attn_out_relayout(ops._ptr(oa), N.JF_BF16, 2, 3, 2, 2, 12, *oa.stride()[:3], ops._ptr(out), ops._stream(oa.device))
    assert rc == N.JF_E_INVALID
    with pytest.raises(ValueError, match="jf_attn_out_relayout"):
        ops.attn_out_relayout(oa, 3, 2, out)


# ------------------------------------------------------------------------------------- 2. plan
def torch_prelude(positions, row_prompt, row_cand, row_len, kv_len_rows, G, S_cur, S_max, T_max, dtype, any_candidates, n_main):
    """Qwen2Model.forward's torch prelude (contiguous layout), line for line: the S_pad-strided bias buffer, slot_main, slot_cand."""
    R, T = positions.shape
    dev = positions.device
    pos = positions.long()
    ar_t = torch.arange(T, device=dev)
    ar_s = torch.arange(S_cur, device=dev)
    kvl = kv_len_rows.long()
    rlen = row_len.long()
    rel = ar_s.view(1, 1, S_cur) - kvl.view(R, 1, 1)
    mask = (rel < 0) | ((rel <= ar_t.view(1, T, 1)) & (rel < rlen.view(R, 1, 1)))
    mask = mask.view(R, 1, 1, T, S_cur).expand(R, 1, G, T, S_cur).reshape(R, 1, G * T, S_cur)
    S_pad = (S_cur + 15) // 16 * 16
    buf = torch.zeros((R, 1, G * T, S_pad), dtype=dtype, device=dev)
    buf[..., :S_cur].masked_fill_(~mask, float("-inf"))
    valid = ar_t.view(1, T) < rlen.view(R, 1)
    main_rows = row_cand < 0
    neg = torch.full_like(pos, -1)
    slot_main = torch.where(valid & main_rows.view(R, 1), row_prompt.long().view(R, 1) * S_max + pos, neg).reshape(-1)
    slot_cand = None
    if n_main is not None:
        RA = int(n_main)
        RB = R - RA
        if RB:
            slot_cand = torch.where(valid[RA:], row_cand[RA:].long().view(RB, 1) * T_max + ar_t.view(1, T), neg[RA:])
            slot_cand = torch.cat([neg[:RA].reshape(-1), slot_cand.reshape(-1)])
    elif any_candidates:
        slot_cand = torch.where(valid & (~main_rows).view(R, 1), row_cand.long().view(R, 1) * T_max + ar_t.view(1, T), neg).reshape(-1)
    return buf, slot_main, slot_cand


PLAN_MODES = {                       # row_cand of the six rows, n_main
    "no_candidates": ([-1] * 6, None),
    "interleaved": ([-1, 0, -1, 2, 1, -1], None),
    "split_RB0": ([-1] * 6, 6),
    "split_RB3": ([-1, -1, -1, 1, 0, 2], 3),
}


@GPU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", list(PLAN_MODES))
def test_plan_matches_the_torch_prelude(mode, dtype):
    cand, n_main = PLAN_MODES[mode]
    R, S_max, T_max, it = 6, 128, 40, INT_OF[dtype]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    row_cand, row_prompt = i32(cand), i32([0, 1, 2, 0, 1, 2])
    any_cand = any(c >= 0 for c in cand)
    for G in (1, 7):
        for T in (1, 8, 33):
            for S_cur in sorted({T, 17, 64, 65}):
                top = max(S_cur - T, 0)
                kv = i32([0, top, top // 2, top, 3 % (top + 1), 0])
                row_len = i32([0, 1, T, T, max(T - 1, 0), (T + 1) // 2])
                pos = (kv.view(R, 1) + torch.arange(T, dtype=torch.int32, device=DEV).view(1, T)).contiguous()
                want = torch_prelude(pos, row_prompt, row_cand, row_len, kv, G, S_cur, S_max, T_max, dtype, any_cand, n_main)
                got = ops.forward_plan(pos.reshape(-1), row_prompt, row_cand, row_len, kv, T, G, S_cur, S_max, T_max, dtype,
                                       want[2] is not None, n_main)
                what = f"G={G} T={T} S_cur={S_cur}"
                assert got[0].shape == want[0].shape and got[0].dtype == dtype, what
                assert torch.equal(got[0].view(it), want[0].view(it)), what          # -inf compared as bits
                assert got[1].dtype == want[1].dtype and torch.equal(got[1], want[1]), what
                assert (got[2] is None) == (want[2] is None), what
                if want[2] is not None:
                    assert got[2].dtype == want[2].dtype and torch.equal(got[2], want[2]), what


# ------------------------------------------------------------------------------------- 3. whole forward, glue on vs off
def two_forwards(model):
    """A prefill on the direct path (row r is cache row r, no candidates), a forward in the loop's split order with two candidate
    rows, one with interleaved candidate rows and one whose rows are a permutation of the cache rows (gathered prefixes); returns
    the four logits and the cache."""
    dev, P = model.device, 3
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    cache = StaticKVCache(model.cfg, P, 64, 2, 8, dev, dtype=model.dtype)
    g = torch.Generator().manual_seed(3)
    lens, T1, T2 = [9, 7, 8], 9, 5
    ids1 = torch.randint(0, model.cfg.vocab_size, (P, T1), generator=g).to(dev)
    pos1 = torch.arange(T1, dtype=torch.int32, device=dev).view(1, T1).expand(P, T1).contiguous()
    l1 = model.forward(ids1, pos1, cache, row_prompt=i32([0, 1, 2]), row_cand=i32([-1] * P), row_len=i32(lens), kv_len_rows=i32([0] * P),
                       any_candidates=False, s_cur=T1)
    kv = i32(lens + [lens[0], lens[2]])
    ids2 = torch.randint(0, model.cfg.vocab_size, (5, T2), generator=g).to(dev)
    pos2 = (kv.view(5, 1) + torch.arange(T2, dtype=torch.int32, device=dev).view(1, T2)).contiguous()
    l2 = model.forward(ids2, pos2, cache, row_prompt=i32([0, 1, 2, 0, 2]), row_cand=i32([-1, -1, -1, 0, 5]), row_len=i32([5, 3, 5, 4, 5]),
                       kv_len_rows=kv, any_candidates=True, s_cur=max(lens) + T2, n_main=3)
    l3 = model.forward(ids2, pos2[[0, 3, 1, 4, 2]].contiguous(), cache, row_prompt=i32([0, 0, 1, 2, 2]), row_cand=i32([-1, 1, -1, 4, -1]),
                       row_len=i32([5, 4, 3, 5, 5]), kv_len_rows=kv[[0, 3, 1, 4, 2]].contiguous(), any_candidates=True, s_cur=max(lens) + T2)
    l4 = model.forward(ids2[:3], pos2[[2, 0, 1]].contiguous(), cache, row_prompt=i32([2, 0, 1]), row_cand=i32([-1] * 3), row_len=i32([5, 5, 2]),
                       kv_len_rows=kv[[2, 0, 1]].contiguous(), any_candidates=False, s_cur=max(lens) + T2, rows_in_place=False)
    return (l1, l2, l3, l4), cache


@GPU
def test_forward_is_the_same_with_and_without_the_glue(monkeypatch):
    cfg = Qwen2Config.tiny()
    model = Qwen2Model(cfg, Qwen2Weights(cfg, torch.device(DEV), dtype=torch.bfloat16, seed=1))
    calls = {"plan": 0, "relayout": 0}
    plan, relayout = ops.forward_plan, ops.attn_out_relayout
    monkeypatch.setattr(ops, "forward_plan", lambda *a, **k: (calls.__setitem__("plan", calls["plan"] + 1), plan(*a, **k))[1])
    monkeypatch.setattr(ops, "attn_out_relayout", lambda *a, **k: (calls.__setitem__("relayout", calls["relayout"] + 1), relayout(*a, **k))[1])
    monkeypatch.setattr(qwen2, "FORWARD_GLUE", True)
    la, ca = two_forwards(model)
    assert calls == {"plan": 4, "relayout": 5 * cfg.num_hidden_layers}, calls     # one copy per layer; split with candidates: two
    monkeypatch.setattr(qwen2, "FORWARD_GLUE", False)
    lb, cb = two_forwards(model)
    assert calls == {"plan": 4, "relayout": 5 * cfg.num_hidden_layers}, calls     # switched off: the torch code ran
    bits = lambda t: t.view(torch.int16)
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(bits(x), bits(y)), f"logits of forward {i}"
    for name in ("k", "v", "ck", "cv"):
        for li, (x, y) in enumerate(zip(getattr(ca, name), getattr(cb, name))):
            assert torch.equal(bits(x), bits(y)), (name, li)
    assert bits(ca.ck[0]).any() and bits(ca.k[0]).any()            # both caches were written


# ------------------------------------------------------------------------------------- 4. the CPU path
class _NoGlueSymbols:
    """The stand-in library with the two new entry points booby-trapped: looking either up fails the test."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        if name in ("jf_attn_out_relayout", "jf_forward_plan"):
            raise AssertionError(f"the CPU forward looked up {name}")
        return getattr(self._inner, name)


def test_cpu_forward_never_looks_up_the_glue_symbols(monkeypatch):
    monkeypatch.setattr(qwen2, "FORWARD_GLUE", True)                # the default: on, and still unused off the GPU
    with use_backend("hostsim") as lib:
        N._LIB = _NoGlueSymbols(lib)                                # use_backend puts the previous library back on exit
        with pytest.raises(AssertionError):
            N.lib().jf_forward_plan
        cfg = Qwen2Config.tiny()
        model = Qwen2Model(cfg, Qwen2Weights(cfg, torch.device("cpu"), dtype=torch.float32, seed=1))
        logits, cache = two_forwards(model)
        assert all(torch.isfinite(l).all() for l in logits) and cache.ck[0].any()
