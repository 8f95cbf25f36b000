"""Lock-step on-policy rollouts: ``generate_rollout_records_batch(seqs, lockstep=True)`` steps every open sequence of a batch in
one forward (``jf_rs_onpolicy_step_batch``).  The contract: per sequence, the records, metrics, final token list, cached length
and draw counts are what the sequential path gives for that sequence ALONE with its own streams — so every expected value here
comes from the oracle (``O.onpolicy_rollout_records_batch``, pinned to the reference's goldens) called once per sequence."""
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from jacobiforcing_amd import _native as N
from jacobiforcing_amd import ops
from jacobiforcing_amd.engine.jacobi_decoding_nongreedy_on_policy import JacobiDecoderNonGreedyOnPolicy
from jacobiforcing_amd.sampling_params import SamplingParams
from oracle import jacobi_oracle as O
from oracle.scripted_model import ScriptedModel

from .backends import device_for, use_backend
from .test_engine_decoder import JDO, TORCH_DTYPES, Harness

ROOT = Path(__file__).resolve().parents[1]
GPU = pytest.mark.gpu
SYMBOL = "jf_rs_onpolicy_step_batch"


# ------------------------------------------------------------------------------------- 1. boundary
def test_the_batch_entry_point_is_declared_exported_and_bound():
    hdr = (ROOT / "include" / "jacobiforcing.h").read_text()
    assert re.search(r"^JF_API\s+int\s+" + SYMBOL + r"\s*\(", hdr, flags=re.M)
    assert SYMBOL in N.EXPORTED_SYMBOLS and "jf_rs_onpolicy_step" in N.EXPORTED_SYMBOLS
    import __graft_entry__ as G
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(G.build_hip())], text=True)
    assert SYMBOL in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert len(N._SIGNATURES[SYMBOL][1]) == 27                       # the header's argument list


# ------------------------------------------------------------------------------------- 3. decoder fuzz vs the oracle
_FILTERS = [(5, None), (None, 0.9), (20, 0.8), (None, 0.5), (3, None), (50, 0.95), (1, None), (None, 0.3)]


def _fuzz_setup(seed):
    rng = np.random.default_rng(31000 + seed)
    V = int(rng.choice([16, 64, 200]))
    B = 1 + seed % 8                                                 # every batch size 1..8 six times over 48 seeds
    eos, pad = V - 1, V - 2
    stop_ids = [eos] if rng.random() < 0.6 else [eos, int(rng.integers(0, V - 2))]
    ldt = "bf16" if seed % 2 else "f32"
    peak = 8.0 if ldt == "f32" else float(rng.choice([3.0, 4.5, 6.0, 8.0]))
    robust = int(rng.choice([0, 30, 60, 80, 100]))
    max_blocks = int(rng.choice([128, 128, 2, 1]))
    T0 = float(rng.choice([1.0, 0.7, 0.4]))
    T1 = float(rng.choice([t for t in (1.0, 0.7, 0.4) if t != T0])) if seed % 4 == 1 else T0     # two temperatures in one batch
    filt = _FILTERS[(seed // 3) % len(_FILTERS)] if seed % 3 == 2 else (None, None)
    same_L = rng.random() < 0.5
    L0 = int(rng.integers(2, 34))
    items = []
    for i in range(B):
        pl = int(rng.integers(1, 40)) if rng.random() < 0.8 else int(rng.integers(250, 262))
        items.append(dict(
            seed=70000 + 29 * seed + i, pl=pl, L=L0 if same_L else int(rng.integers(2, 34)), mt=int(rng.integers(1, 70)),
            eos_pos=None if rng.random() < 0.45 else pl + int(rng.integers(0, 40)), T=T1 if i % 2 else T0,
            # seeds 5, 11, ... plant the filters on every other request only: rows of one temperature fall into two groups
            filt=filt if (seed % 6 != 5 or i % 2 == 0) else (None, None),
            unis=[float(x) for x in (rng.integers(0, 1 << 24, size=2048) / float(1 << 24))],
            multi=[float(x) for x in (rng.integers(0, 1 << 24, size=2048) / float(1 << 24))]))
    return dict(V=V, eos=eos, pad=pad, stop_ids=stop_ids, ldt=ldt, peak=peak, robust=robust, max_blocks=max_blocks, items=items)


def _taker(arr, cur, name):
    def f():
        v = arr[cur[name] % len(arr)]
        cur[name] += 1
        return v
    return f


def _oracle_alone(cfg, i, it, model):
    """sequence i of the batch, alone, with its own streams: (records, metrics, oracle sequence, [uniforms, multinomial], inits)"""
    ldt = cfg["ldt"]
    oseq = O.OracleSeq(model.prompt(), it["L"], it["mt"], max_iters=cfg["max_blocks"])
    cur = {"u": 0, "m": 0}
    inits = O.CounterStream(9000 + it["seed"])

    def ofwd(ss, drafts):
        lg = model.logits_rows(ss[0].token_ids[:-1], [drafts[0]])[0][:-1]
        return [O.bf16_round(lg) if ldt == "bf16" else lg]
    rec, met = O.onpolicy_rollout_records_batch(ofwd, [oseq], it["T"], cfg["stop_ids"], cfg["pad"], cfg["V"], O.ScriptedRandom(inits),
                                                _taker(it["unis"], cur, "u"), _taker(it["multi"], cur, "m"), data_ids=[f"data_{i}"],
                                                logits_dtype=ldt, top_k=it["filt"][0], top_p=it["filt"][1])
    return rec[0], met[0], oseq, [cur["u"], cur["m"]], inits.k


def _build(cfg, backend, **dec_kw):
    dev = device_for(backend)
    H = Harness(cfg["V"], dev, TORCH_DTYPES[cfg["ldt"]])
    stop = cfg["stop_ids"] if len(cfg["stop_ids"]) > 1 else cfg["eos"]
    kw = dict(forward_step=lambda s, d: H.forward_step_batch([s], d), forward_step_batch=H.forward_step_batch)
    kw.update(dec_kw)
    dec = JacobiDecoderNonGreedyOnPolicy(H.bm, eos_token_id=stop, pad_token_id=cfg["pad"], vocab_size=cfg["V"],
                                         device=torch.device(dev), **kw)
    seqs, models = [], []
    for it in cfg["items"]:
        m = ScriptedModel(cfg["V"], it["seed"], cfg["robust"], it["pl"], eos_id=cfg["eos"], eos_pos=it["eos_pos"],
                          reserved=(cfg["pad"],), peak=cfg["peak"])
        sp = SamplingParams(temperature=it["T"], max_tokens=it["mt"], decode_strategy="jacobi", jacobi_block_len=it["L"],
                            jacobi_max_iterations=cfg["max_blocks"], jacobi_on_policy=True)
        if it["filt"][0] is not None:
            sp.top_k = it["filt"][0]
        if it["filt"][1] is not None:
            sp.top_p = it["filt"][1]
        seqs.append(H.add(m, sp, None))
        models.append(m)
    return H, dec, seqs, models


def _run_fuzz(seed, backend):
    cfg = _fuzz_setup(seed)
    with use_backend(backend):
        H, dec, seqs, models = _build(cfg, backend)
        inits = [O.CounterStream(9000 + it["seed"]) for it in cfg["items"]]
        dec.set_streams_per_sequence([O.ScriptedRandom(s) for s in inits], [it["unis"] for it in cfg["items"]],
                                     [it["multi"] for it in cfg["items"]])
        got, gmet = dec.generate_rollout_records_batch(seqs, return_metrics=True, lockstep=True)
        assert len(got) == len(gmet) == len(seqs)
        for i, (it, m) in enumerate(zip(cfg["items"], models)):
            want, wmet, oseq, cursors, n_inits = _oracle_alone(cfg, i, it, m)
            assert got[i] == want, (seed, i)
            assert gmet[i] == wmet, (seed, i)
            assert seqs[i].token_ids == oseq.token_ids and seqs[i].num_cached_tokens == oseq.num_cached_tokens == len(seqs[i])
            assert dec.cursors_per_sequence[i] == cursors and inits[i].k == n_inits, (seed, i)
        assert dec._batch_stepper.cursors.cpu().tolist() == dec.cursors_per_sequence     # the device's cursors, never re-uploaded
    return cfg, H, got


@pytest.mark.parametrize("seed", range(48))
def test_lockstep_rollouts_equal_every_sequence_decoded_alone(seed):
    _run_fuzz(seed, "hostsim")


def test_the_fuzz_sweep_covers_what_it_claims():
    cfgs = [_fuzz_setup(s) for s in range(48)]
    assert {len(c["items"]) for c in cfgs} == set(range(1, 9))
    Ls = {it["L"] for c in cfgs for it in c["items"]}
    assert min(Ls) == 2 and max(Ls) == 33
    assert {len(c["stop_ids"]) for c in cfgs} == {1, 2} and {c["ldt"] for c in cfgs} == {"f32", "bf16"}
    assert {it["T"] for c in cfgs for it in c["items"]} == {1.0, 0.7, 0.4}
    assert sum(any(it["filt"] != (None, None) for it in c["items"]) for c in cfgs) == 16
    assert sum(len({it["T"] for it in c["items"]}) == 2 for c in cfgs) >= 8
    assert sum(len({it["L"] for it in c["items"]}) > 1 for c in cfgs) >= 8
    assert any(it["eos_pos"] is not None for c in cfgs for it in c["items"])


@GPU
@pytest.mark.parametrize("seed", [3 * k + k % 3 for k in range(16)])
def test_lockstep_rollouts_equal_every_sequence_decoded_alone_on_the_gpu(seed):
    """16 of the sweep's seeds through the HIP kernels: both dtypes, mixed temperatures, top_k / top_p on every third one"""
    _run_fuzz(seed, "hip")


# ------------------------------------------------------------------------------------- 4. the padding argument
def test_scripted_logits_do_not_see_a_rows_tail():
    """Right-padding a draft leaves the logits of the positions in front of the padding unchanged (the model is causal):
    lock-step pads ragged rows to the longest of their group and relies on it."""
    m = ScriptedModel(64, 4711, 60, 9, eos_id=63, eos_pos=None, reserved=(62,), peak=4.5)
    committed = m.prompt()[:-1]
    row = [m.prompt()[-1], 5, 17, 3, 40]
    short = m.logits_rows(committed, [row])[0]
    for tail in ([62] * 7, [1, 2, 3], [62]):
        padded = m.logits_rows(committed, [row + tail])[0]
        assert padded.shape[0] == len(row) + len(tail)
        assert np.array_equal(padded[:len(row)], short)


# ------------------------------------------------------------------------------------- 5. batching really happens
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_one_forward_carries_every_open_row(seed):
    rng = np.random.default_rng(500 + seed)
    V, B = 64, 6
    items = [dict(seed=81000 + 7 * seed + i, pl=int(rng.integers(2, 30)), L=int(rng.choice([5, 8, 16])), mt=int(rng.integers(4, 50)),
                  eos_pos=None, T=0.7, filt=(None, None),
                  unis=[float(x) for x in (rng.integers(0, 1 << 24, size=2048) / float(1 << 24))],
                  multi=[float(x) for x in (rng.integers(0, 1 << 24, size=2048) / float(1 << 24))]) for i in range(B)]
    items[2]["eos_pos"] = items[2]["pl"] + 6                       # one sequence stops early
    cfg = dict(V=V, eos=V - 1, pad=V - 2, stop_ids=[V - 1], ldt="f32", peak=8.0, robust=60, max_blocks=128, items=items)
    with use_backend("hostsim"):
        H, dec, seqs, models = _build(cfg, "hostsim")
        dec.set_streams_per_sequence([O.ScriptedRandom(O.CounterStream(9000 + it["seed"])) for it in items],
                                     [it["unis"] for it in items], [it["multi"] for it in items])
        dec.generate_rollout_records_batch(seqs, lockstep=True)
        per_block = []                                              # per sequence: forwards of block 0, 1, ... (from the oracle)
        for i, (it, m) in enumerate(zip(items, models)):
            rec = _oracle_alone(cfg, i, it, m)[0]
            nf = [rec[k]["num_forwards"] for k in sorted(rec)]
            per_block.append([b - a for a, b in zip([0] + nf[:-1], nf)])
        want = []
        for k in range(max(len(p) for p in per_block)):
            fk = {i: p[k] for i, p in enumerate(per_block) if k < len(p)}
            want += [[i for i in sorted(fk) if fk[i] > j] for j in range(max(fk.values()))]
        assert [t["seq_idx"] for t in H.trace] == want
        assert len(H.trace) == sum(max(p[k] for p in per_block if k < len(p)) for k in range(max(len(p) for p in per_block)))
        assert len(H.trace) < sum(sum(p) for p in per_block)        # fewer forwards than one per sequence and step
        assert [(g, l) for g, l, _ in dec.lockstep_forwards] == [(len(t["seq_idx"]), len(t["draft"][0]) - 1) for t in H.trace]
        # the default path on the same batch: one row per forward, sequence after sequence, as before
        H2, dec2, seqs2, _ = _build(cfg, "hostsim")
        dec2.set_streams(O.ScriptedRandom(O.CounterStream(1)), items[0]["unis"], items[0]["multi"])
        _, met = dec2.generate_rollout_records_batch(seqs2, return_metrics=True)
        assert all(len(t["seq_idx"]) == 1 for t in H2.trace) and len(H2.trace) == sum(int(m_["num_forwards"]) for m_ in met)


# ------------------------------------------------------------------------------------- 6. golden replay
_SINGLE = ["jdo_single_T1", "jdo_maxblocks2", "jdo_hot_T2", "jdo2_bf16_single_T1", "jdo2_bf16_hot_T2", "jdo4_bf16_V64_k10_p08"]
_BY_NAME = {c["name"]: c for c in JDO}


def _golden_decoder(case, backend):
    p = case["params"]
    dev = device_for(backend)
    H = Harness(p["vocab"], dev, TORCH_DTYPES[p.get("logits_dtype", "f32")])
    stop = p["stop_ids"] if len(p["stop_ids"]) > 1 else p["eos_id"]
    dec = JacobiDecoderNonGreedyOnPolicy(H.bm, forward_step=lambda s, d: H.forward_step_batch([s], d),
                                         forward_step_batch=H.forward_step_batch, eos_token_id=stop, pad_token_id=p["pad_id"],
                                         vocab_size=p["vocab"], device=torch.device(dev))
    seqs = []
    for d in case["seqs"]:
        sp = SamplingParams(temperature=p["temperature"], max_tokens=p["max_tokens"], decode_strategy="jacobi",
                            jacobi_block_len=p["block_len"], jacobi_max_iterations=p["max_blocks"], jacobi_on_policy=True)
        for k in ("top_k", "top_p"):
            if k in p:
                setattr(sp, k, p[k])
        seqs.append(H.add(ScriptedModel.from_dict(d["model"]), sp, None))
    streams = tuple(O.CounterStream(p["rng_seed"] * 5 + k) for k in (1, 2, 3))
    return H, dec, seqs, streams


@pytest.mark.parametrize("name", _SINGLE)
def test_single_sequence_goldens_replay_in_lockstep(name):
    """The reference's single-sequence records: for one sequence the per-sequence streams ARE the shared stream and nothing is
    padded, so lock-step must give the reference's records, metrics, draw counts and forward inputs."""
    case = _BY_NAME[name]
    assert len(case["seqs"]) == 1
    with use_backend("hostsim"):
        H, dec, seqs, (inits, unis, multi) = _golden_decoder(case, "hostsim")
        dr = case["draws"]
        dec.set_streams_per_sequence([O.ScriptedRandom(inits)], [[unis.uniform() for _ in range(dr["uniforms"] + 64)]],
                                     [[multi.uniform() for _ in range(dr["multinomial"] + 64)]])
        records, metrics = dec.generate_rollout_records_batch(seqs, return_metrics=True, lockstep=True)
        assert [{str(k): v for k, v in r.items()} for r in records] == case["records"]
        assert metrics == case["metrics"]
        cur = dec.cursors_per_sequence[0]
        assert dict(inits=inits.k, uniforms=cur[0], multinomial=cur[1]) == case["draws"]
        for s, f in zip(seqs, case["final"]):
            assert s.token_ids == f["token_ids"] and s.num_cached_tokens == f["num_cached_tokens"]
        assert [(t["draft"], t["seq_lens"]) for t in H.trace] == [(t["draft"], t["seq_lens"]) for t in case["forwards"]]


# ------------------------------------------------------------------------------------- 7. the default is untouched
def test_lockstep_is_opt_in():
    for fn in (JacobiDecoderNonGreedyOnPolicy.generate_rollout_records_batch, JacobiDecoderNonGreedyOnPolicy.generate_rollout_records):
        assert inspect.signature(fn).parameters["lockstep"].default is False
    multi = [c for c in JDO if len(c["seqs"]) > 1][:2]
    assert len(multi) == 2
    for case in multi:
        with use_backend("hostsim"):
            H, dec, seqs, (inits, unis, mult) = _golden_decoder(case, "hostsim")
            dr = case["draws"]
            dec.set_streams(O.ScriptedRandom(inits), [unis.uniform() for _ in range(dr["uniforms"] + 64)],
                            [mult.uniform() for _ in range(dr["multinomial"] + 64)])
            records = dec.generate_rollout_records_batch(seqs, lockstep=False)
            assert [{str(k): v for k, v in r.items()} for r in records] == case["records"]
            assert dict(inits=inits.k, uniforms=dec._cur[0], multinomial=dec._cur[1]) == case["draws"]


# ------------------------------------------------------------------------------------- 8. errors
def test_lockstep_errors():
    cfg = _fuzz_setup(3)
    with use_backend("hostsim"):
        H, dec, seqs, _ = _build(cfg, "hostsim", forward_step_batch=None)
        with pytest.raises(ValueError, match="forward_step_batch"):
            dec.generate_rollout_records_batch(seqs, lockstep=True)
        with pytest.raises(ValueError, match="forward_step_batch"):
            dec.generate_rollout_records(seqs[0], lockstep=True)
        H, dec, seqs, _ = _build(cfg, "hostsim")
        dec.forward_step_batch = lambda ss, d: H.forward_step_batch(ss, d)[:, :-1]
        B, Lm = len(seqs), max(min(it["L"], it["mt"]) for it in cfg["items"])
        with pytest.raises(ValueError, match=re.escape(f"forward must return logits [{B}, {Lm}, vocab], got ")):
            dec.generate_rollout_records_batch(seqs, lockstep=True)
        H, dec, seqs, _ = _build(cfg, "hostsim")
        dec.set_streams_per_sequence([None], [[0.5]], [[0.5]])
        with pytest.raises(ValueError, match="set_streams_per_sequence"):
            dec.generate_rollout_records_batch(seqs, lockstep=True)
        with pytest.raises(ValueError):
            dec.set_streams_per_sequence([None, None], [[0.5]], [[0.5]])


def test_a_row_that_padding_would_push_over_the_cache_bound_is_stepped_alone():
    """With a bound on the positions a forward may reach, a short row is not padded past it: it gets a forward of its own (which
    fits, as it does on the sequential path) and the records stay what they are."""
    rng = np.random.default_rng(77)
    mk = lambda i, pl, L, mt: dict(seed=88000 + i, pl=pl, L=L, mt=mt, eos_pos=None, T=1.0, filt=(None, None),
                                   unis=[float(x) for x in (rng.integers(0, 1 << 24, size=512) / float(1 << 24))],
                                   multi=[float(x) for x in (rng.integers(0, 1 << 24, size=512) / float(1 << 24))])
    items = [mk(0, 40, 4, 4), mk(1, 10, 16, 16)]                   # sequence 0 ends at 44 positions; padded to 16 it would reach 56
    cfg = dict(V=64, eos=63, pad=62, stop_ids=[63], ldt="f32", peak=8.0, robust=60, max_blocks=1, items=items)
    with use_backend("hostsim"):
        H, dec, seqs, models = _build(cfg, "hostsim")
        dec.max_forward_positions = 45
        dec.set_streams_per_sequence([O.ScriptedRandom(O.CounterStream(9000 + it["seed"])) for it in items],
                                     [it["unis"] for it in items], [it["multi"] for it in items])
        got = dec.generate_rollout_records_batch(seqs, lockstep=True)
        for i, (it, m) in enumerate(zip(items, models)):
            assert got[i] == _oracle_alone(cfg, i, it, m)[0]
        assert all(sl + len(d) - 1 <= 45 for t in H.trace for sl, d in zip(t["seq_lens"], t["draft"]))
        assert all(len(t["seq_idx"]) == 1 for t in H.trace if 0 in t["seq_idx"])


# ------------------------------------------------------------------------------------- 9 + 11. the kernels at the real vocabulary
def _planted_batch(dtype):
    """G = 4 ragged sequences at V = 152064: 0 accepts all 12, 1 rejects at row 0, 2 (one row) commits a stop id, 3 rejects at
    row 4 and re-drafts rows 5..8.  Streams of different lengths, cursors that do not start at 0."""
    G, Lm, V, stop = 4, 12, 152064, 3
    n_rows = [12, 7, 1, 9]
    g = torch.Generator().manual_seed(47)
    proposed = torch.randint(4, V, (G, Lm), generator=g)
    logits = torch.randn(G, Lm, V, generator=g) * 0.5
    boost = float(np.log(0.8 / 0.2 * (V - 1)))
    proposed[2, 0] = stop
    for q in range(G):
        proposed[q, n_rows[q]:] = 0                                  # padding (never read by the step)
        logits[q, torch.arange(n_rows[q]), proposed[q, :n_rows[q]]] = boost
    logits[1, 0, proposed[1, 0]] = 0.0
    logits[3, 4, proposed[3, 4]] = 0.0
    lens = [(64, 80), (48, 96), (32, 40), (72, 56)]
    cur0 = [[2, 5], [60, 90], [31, 7], [0, 50]]                      # sequence 1's windows wrap around
    us, ms = [], []
    for q, (lu, lm_) in enumerate(lens):
        u = torch.randint(0, 1 << 24, (lu,), generator=g).float() / float(1 << 24)
        for t in range(n_rows[q]):
            u[(cur0[q][0] + t) % lu] = 0.01                           # every test that is reached accepts unless p is tiny
        us.append(u.numpy())
        ms.append((torch.randint(0, 1 << 24, (lm_,), generator=g).float() / float(1 << 24)).numpy())
    return dict(G=G, Lm=Lm, V=V, stop=stop, n_rows=n_rows, proposed=proposed, logits=logits.to(dtype), us=us, ms=ms, cur0=cur0)


def _step_planted(backend, b, temperature, top_k=0, top_p=0.0):
    with use_backend(backend):
        dev = device_for(backend)
        st = ops.OnPolicyBatchStepper(b["G"], max(16, b["Lm"]), dev, b["us"], b["ms"], [b["stop"]])
        st.cursors.copy_(torch.tensor(b["cur0"], dtype=torch.int64))
        rows, cm, rd = st.step(b["proposed"].to(dev), b["n_rows"], b["logits"].to(dev), temperature, list(range(b["G"])), top_k, top_p)
        return rows, cm, rd, st.cursors.cpu().tolist(), st.packed.cpu()


def _assert_planted(b, hip, sim):
    rows_h, cm_h, rd_h, cur_h, pk_h = hip
    rows_o, cm_o, rd_o, cur_o, _ = sim
    R = b["n_rows"]
    assert [r["n_committed"] for r in rows_o] == [12, 1, 1, 5]
    assert [r["reject_pos"] for r in rows_o] == [-1, 0, -1, 4] and [r["stop_hit"] for r in rows_o] == [0, 0, 1, 0]
    assert [r["n_redraft"] for r in rows_o] == [0, R[1] - 1, 0, R[3] - 5] and [r["n_uniforms"] for r in rows_o] == [12, 1, 1, 5]
    assert rows_h == rows_o and cm_h == cm_o and cur_h == cur_o
    for q in range(b["G"]):
        n = rows_o[q]["n_committed"]
        assert len(rd_h[q]) == R[q] and rd_h[q][n:] == rd_o[q][n:]
    assert cur_o == [[c[0] + r["n_uniforms"], c[1] + r["n_bonus_draws"] + r["n_redraft"]] for c, r in zip(b["cur0"], rows_o)]
    assert int(pk_h[:b["G"] * b["Lm"]].abs().sum()) == 0


@GPU
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_rs_onpolicy_step_batch_at_the_real_vocabulary(dtype, temperature):
    """jf_rs_probs + jf_rs_onpolicy_step_batch on a ragged [4, 12] rectangle at V = 152064 against the stand-in (the oracle's
    single-sequence step, sequence by sequence): records, committed tokens, re-drafted rows, every cursor, packed re-zeroed."""
    b = _planted_batch(dtype)
    _assert_planted(b, _step_planted("hip", b, temperature), _step_planted("hostsim", b, temperature))


@GPU
def test_rs_onpolicy_step_batch_with_top_k_and_top_p_at_the_real_vocabulary():
    b = _planted_batch(torch.bfloat16)
    _assert_planted(b, _step_planted("hip", b, 0.7, 50, 0.9), _step_planted("hostsim", b, 0.7, 50, 0.9))


@GPU
def test_a_row_count_outside_the_rectangle_is_refused_by_the_kernel():
    """n_rows is a device array the host cannot check: the accept launch marks such a sequence (n_committed = -1) and touches
    nothing else of it — its cursors stay, its neighbours are stepped."""
    b = _planted_batch(torch.float32)
    with use_backend("hip"):
        dev = device_for("hip")
        st = ops.OnPolicyBatchStepper(b["G"], 16, dev, b["us"], b["ms"], [b["stop"]])
        st.cursors.copy_(torch.tensor(b["cur0"], dtype=torch.int64))
        G, Lm, V = b["G"], b["Lm"], b["V"]
        flat = b["logits"].to(dev).reshape(G * Lm, V)
        prop = b["proposed"].to(dev).contiguous()
        nr = torch.tensor([12, 0, 1, 13], dtype=torch.int32, device=dev)
        lib = N.lib()
        st.ws = ops._grown(st.ws, int(lib.jf_rs_workspace_bytes(G * Lm, V)))
        p = ops._ptr
        N.check(lib.jf_rs_probs(p(flat), N.JF_F32, G * Lm, V, V, p(prop), 1.0, p(st.p_draft), p(st.row_max), p(st.row_sumexp),
                                p(st.packed), p(st.ws), st.ws.numel() * 4, ops._stream(torch.device(dev))), "jf_rs_probs")
        cm = torch.full((G, Lm), -7, dtype=torch.int64, device=dev)
        rd = torch.full((G, Lm), -7, dtype=torch.int64, device=dev)
        rows = torch.zeros((G, N.OP_ROW_INTS), dtype=torch.int32, device=dev)
        N.check(lib.jf_rs_onpolicy_step_batch(p(flat), N.JF_F32, V, V, p(prop), p(nr), G, Lm, p(st.p_draft), p(st.row_max),
                                              p(st.row_sumexp), p(st.packed), 1.0, p(st.stop_ids), 1, p(st.u_stream), p(st.m_stream),
                                              p(st.stream_off), p(st.stream_len), p(st.cursors), p(cm), p(rd), p(rows), p(st.step_ws),
                                              st.step_ws.numel() * 8, None, ops._stream(torch.device(dev))), SYMBOL)
        torch.cuda.synchronize()
        rows, cur = rows.cpu().tolist(), st.cursors.cpu().tolist()
        assert [r[0] for r in rows] == [12, -1, 1, -1]
        assert cur[1] == b["cur0"][1] and cur[3] == b["cur0"][3] and cur[0][0] == b["cur0"][0][0] + 12
        assert (cm[1] == -7).all() and (cm[3] == -7).all() and (rd[1] == -7).all() and (rd[3] == -7).all()
        assert int(st.packed[:G * Lm].abs().sum()) == 0


# ------------------------------------------------------------------------------------- 12. the two entry points agree
def _small_batch(n_rows, reject_at, stop_at, lens, cur0, seed):
    """Ragged sequences at V = 64, float32, T = 1: every proposed id holds ~0.78 of its row and every uniform is below 0.5, so
    a test accepts unless it is planted: ``reject_at`` {g: t} gives row t's proposed id ~1e-14, ``stop_at`` {g: t} proposes the
    stop id there.  ``lens`` [(uniforms, multinomial)] and ``cur0`` per sequence; a stream shorter than its sequence wraps."""
    G, Lm, V, stop = len(n_rows), max(n_rows), 64, 3
    g = torch.Generator().manual_seed(seed)
    proposed = torch.randint(4, V, (G, Lm), generator=g)
    logits = torch.randn(G, Lm, V, generator=g) * 0.5
    for q, t in stop_at.items():
        proposed[q, t] = stop
    for q in range(G):
        proposed[q, n_rows[q]:] = 0                                  # padding (never read by the step)
        logits[q, torch.arange(n_rows[q]), proposed[q, :n_rows[q]]] = float(np.log(4.0 * (V - 1)))
    for q, t in reject_at.items():
        logits[q, t, proposed[q, t]] = -30.0
    us = [(torch.randint(0, 1 << 23, (lu,), generator=g).float() / float(1 << 24)).numpy() for lu, _ in lens]
    ms = [(torch.randint(0, 1 << 24, (lm_,), generator=g).float() / float(1 << 24)).numpy() for _, lm_ in lens]
    return dict(G=G, Lm=Lm, V=V, stop=stop, n_rows=list(n_rows), proposed=proposed, logits=logits, us=us, ms=ms, cur0=cur0)


def _step_alone(backend, b, q, temperature, top_k=0, top_p=0.0):
    """sequence q of the batch through the single-sequence entry point: its rows, its stream window, its starting cursors"""
    with use_backend(backend):
        dev = device_for(backend)
        R = b["n_rows"][q]
        st = ops.OnPolicyStepper(max(16, R), dev, b["us"][q], b["ms"][q], [b["stop"]])
        row, cm, rd = st.step(b["proposed"][q, :R].to(dev), b["logits"][q, :R].to(dev), temperature, b["cur0"][q], top_k, top_p)
        return row, cm, rd, st.cursors.cpu().tolist(), st.packed.cpu()


def _assert_entries_agree(b, batch, alone):
    rows, cm, rd, cur, pk = batch
    assert int(pk[:b["G"] * b["Lm"]].abs().sum()) == 0
    for q, (row1, cm1, rd1, cur1, pk1) in enumerate(alone):
        R, n = b["n_rows"][q], rows[q]["n_committed"]
        assert len(row1) == N.OP_ROW_INTS == 8 and row1 == rows[q], q
        assert len(cm1) == n and cm1 == cm[q], q
        assert len(rd1) == len(rd[q]) == R and rd1[n:] == rd[q][n:], q
        assert cur1 == cur[q], q
        assert int(pk1[:R].abs().sum()) == 0


def _p_draft_on_the_gpu(b):
    """jf_rs_probs once on the whole rectangle (float32, T = 1): the kernel's own float32 probability of every proposed id"""
    with use_backend("hip"):
        dev = torch.device(device_for("hip"))
        n, V = b["G"] * b["Lm"], b["V"]
        flat, prop = b["logits"].to(dev).reshape(n, V), b["proposed"].to(dev).contiguous()
        lib, p = N.lib(), ops._ptr
        p_draft, row_max, row_sumexp = (torch.zeros((n,), dtype=torch.float32, device=dev) for _ in range(3))
        packed = ops.new_packed(n, dev)
        ws = torch.zeros((int(lib.jf_rs_workspace_bytes(n, V)) // 4 + 4,), dtype=torch.float32, device=dev)
        N.check(lib.jf_rs_probs(p(flat), N.JF_F32, n, V, V, p(prop), 1.0, p(p_draft), p(row_max), p(row_sumexp), p(packed), p(ws),
                                ws.numel() * 4, ops._stream(dev)), "jf_rs_probs")
        return p_draft.cpu().view(b["G"], b["Lm"])


def _agree_chunk_boundaries():
    """(a) row counts around the 64-lane ballot chunk and the 256-thread loop: 0 accepts its one row, 1 rejects at row 0, 2
    commits a stop id at row 40, 3 rejects at row 64 (the first lane of the second chunk), 4 accepts all 257 from a uniform
    stream of 100 (it wraps twice; so does sequence 1's multinomial stream of 40 under its 62 re-drafts)."""
    b = _small_batch([1, 63, 64, 65, 257], {1: 0, 3: 64}, {2: 40}, [(32, 32), (96, 40), (128, 64), (80, 72), (100, 48)],
                     [[7, 3], [90, 35], [11, 60], [79, 1], [33, 47]], 61)
    return b, 1.0, 0, 0.0, dict(n_committed=[1, 1, 41, 65, 257], reject_pos=[-1, 0, -1, 64, -1], stop_hit=[0, 0, 1, 0, 0])


def _agree_real_vocabulary():
    """(b) the planted batch at V = 152064 in bfloat16 with a temperature and both filters"""
    return _planted_batch(torch.bfloat16), 0.7, 50, 0.9, None


def _agree_outside_lds():
    """(c) more than RS_OP_STAGE = 2048 rows per sequence: the accept entries are recomputed per ballot and resolved tests go
    through the patch table.  Sequence 0 rejects at row 2048 (one re-draft behind it); in sequence 1 the uniforms of three
    tests EQUAL the kernel's float32 probability of their row — the tests a kernel may mark undecided and resolve exactly."""
    b = _small_batch([2050, 2049], {0: 2048}, {}, [(4096, 4096), (4096, 4096)], [[5, 9], [17, 2]], 67)
    pd = _p_draft_on_the_gpu(b)
    for t in (5, 700, 2047):
        b["us"][1][b["cur0"][1][0] + t] = float(pd[1, t])
    return b, 1.0, 0, 0.0, dict(reject_pos_0=2048)


@GPU
@pytest.mark.parametrize("case", [_agree_chunk_boundaries, _agree_real_vocabulary, _agree_outside_lds],
                         ids=["chunk_boundaries", "real_vocabulary", "outside_lds"])
def test_the_single_and_the_batch_entry_point_agree(case):
    """One jf_rs_onpolicy_step_batch call on a ragged batch against one jf_rs_onpolicy_step call per sequence (its rows, stream
    window and starting cursors): the eight ints of every record, committed[:n], redraft[n:R], both cursors afterwards and
    packed re-zeroed are identical; at V = 64 both are also what the host stand-in gives."""
    b, temperature, top_k, top_p, planted = case()
    batch = _step_planted("hip", b, temperature, top_k, top_p)
    alone = [_step_alone("hip", b, q, temperature, top_k, top_p) for q in range(b["G"])]
    _assert_entries_agree(b, batch, alone)
    if planted is None:
        return
    sim = _step_planted("hostsim", b, temperature, top_k, top_p)
    if "reject_pos_0" in planted:
        assert sim[0][0]["reject_pos"] == planted["reject_pos_0"] and sim[0][0]["n_redraft"] == 1
    else:
        for k, want in planted.items():
            assert [r[k] for r in sim[0]] == want, k
    _assert_entries_agree(b, sim, alone)
