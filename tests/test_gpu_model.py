"""GPU parity, model level: the device-resident decode path (Tier-2 C ABI) vs the oracle's restatement of
AbstractModel.generate(), on seeded synthetic JQ4 Llama models.

Tolerances.  BASELINE.json: token ids at temperature 0 bit-exact, logits within 1e-2 on the Q8 (I8-activation) path.
What is achievable is bounded by the reference's own arithmetic: the Q8 activation quantizer
(PanamaTensorOperations.java:1684-1723) is a step function, and the float summation order of every GEMV differs
between any two providers (Panama's reduceLanes order is itself unspecified).  Measured on these random-weight models
(tools/dbg_traj.py): GPU and oracle agree to ~2e-7 until the first I8 code flips, then the difference settles at a
noise floor of ~1e-2 absolute on O(1) logits (every flip moves a GEMV output by scale/127*|w|, and a perturbed
activation row flips ~10% of the next quantizer's codes).  So the tests hold:
  * stage taps: every layer is fed the GPU's own input rows (per-layer teacher forcing), 1e-4 relative for the taps
    upstream of the layer's second quantizer; the bit-exact / per-layer checks proper live in tests/test_gpu_parity.py
    (strict-order mode: zero tolerance at every layer; fast kernels: every layer in isolation);
  * free-running multi-layer outputs (flips cascade through layers): TRUNK_TOL relative, logits LOGIT_TOL = 4e-2
    absolute at every teacher-forced step, mean |diff| <= 5e-3;
  * token ids: bit-exact wherever the oracle's own decision margin exceeds LOGIT_TOL (a smaller margin is a coin
    flip between ANY two correct implementations; in strict-order mode they are simply bit-exact)."""
import os

import numpy as np
import pytest

from jlama_amd import _native as _N

pytestmark = pytest.mark.gpu
FLIP_ROW = 5e-2   # one tipped Q8 code moves a row of a single-layer model by about one code step of its scale

LOGIT_TOL = 4e-2
TRUNK_TOL = 4e-2   # relative to the row's max |x|


def _pair(cfg, seed, oracle, layer_range=None):
    from jlama_amd import synthetic as S
    from jlama_amd.model import HipLlamaModel
    w = S.make_weights(cfg, seed=seed, quantize=oracle.q4_quantize)   # compiled quantizer, bit-equal to jq4 (test_oracle.py)
    return HipLlamaModel(cfg, w, layer_range=layer_range), oracle.OracleModel(cfg, w, layer_range=layer_range), w


def _rel(got, want):
    return np.abs(got - want).max() / (np.abs(want).max() + 1e-30)


@pytest.mark.parametrize("cfgname", ["TINY", "SMALL"])
def test_stage_taps_single_token(gpu, oracle, cfgname):
    """DebugSupport-named stage taps of EVERY layer at 1e-4: the oracle's layer l is fed the GPU's own input rows of
    layer l (teacher forcing), so no layer inherits quantizer flips from the ones before it."""
    from jlama_amd import synthetic as S
    cfg = dict(getattr(S, cfgname))
    hm, om, w = _pair(cfg, 0, oracle)
    prompt = S.prompt_tokens(cfg, n=9, seed=5)
    E, A = cfg["embedding_length"], cfg["n_heads"] * cfg["head_size"]
    KV = cfg["n_kv_heads"] * cfg["head_size"]
    for layer in range(cfg["n_layers"]):
        hs2 = hm.session(64)
        hs2.set_tap_layer(layer)
        om_l = oracle.OracleModel(cfg, w, layer_range=(layer, layer + 1))
        os2 = om_l.session()
        os2.set_tap_layer(layer)
        for i, t in enumerate(prompt):
            hs2.forward([t], i, want_output=False)
            x_in = hs2.tap("input_emb", E)
            os2.forward(None, i, x=x_in.reshape(1, E))
        for name, n, tol in [("input_emb", E, 0.0), ("query", A, 1e-4), ("key", KV, 1e-4), ("value", KV, 1e-4),
                             ("query+rope", A, 1e-4), ("key+rope", KV, 1e-4), ("after_attention", A, 1e-4),
                             ("post_ff_res", E, 3e-3)]:   # post_ff_res sits behind three more quantizers of this layer
            got, want = hs2.tap(name, n), os2.tap(name, n)
            if layer == 0 and name == "input_emb":
                om0 = om.session()
                om0.set_tap_layer(0)
                om0.forward([prompt[-1]], 0)
                np.testing.assert_array_equal(got, om0.tap(name, n))  # Q4 embedding row dequantization is exact
            assert _rel(got, want) <= tol, (layer, name, _rel(got, want))


def test_prefill_logits_and_greedy_tokens(gpu, oracle):
    from jlama_amd import synthetic as S
    cfg = dict(S.SMALL)
    hm, om, _ = _pair(cfg, 1, oracle)
    prompt = S.prompt_tokens(cfg, n=40, seed=11)   # 41 rows > ctxPerPage => crosses KV pages
    hs, os_ = hm.session(160), om.session()
    assert hs.page_info() == os_.page_info()
    out_h = hs.batch_forward(prompt, 0)
    out_o = os_.forward(prompt, 0)
    assert _rel(out_h, out_o) <= TRUNK_TOL
    tok_h, logits_h = hs.sample(0.0, 0.5, want_logits=True)
    tok_o, logits_o = om.sample(out_o[-1])
    assert np.abs(logits_h - logits_o).max() <= LOGIT_TOL
    # greedy decode, teacher-forced with the GPU's own ids so both KV caches see the same inputs at every step:
    #  * logits within LOGIT_TOL at EVERY step (see the module docstring);
    #  * token ids bit-exact wherever the decision is meaningful, i.e. the oracle's margin between its argmax and the
    #    GPU's pick exceeds the logit tolerance (random-weight models produce occasional near-ties).
    n_gen = 100
    tok = tok_h
    assert tok_h == tok_o or logits_o.max() - logits_o[tok_h] <= LOGIT_TOL
    exact, mean_diff = 0, []
    for i in range(n_gen):
        pos = prompt.size + i
        nxt_h = hs.decode_step(tok, pos)
        lh = hs.logits()
        xo = os_.forward([tok], pos)
        nxt_o, lo = om.sample(xo[-1])
        assert np.abs(lh - lo).max() <= LOGIT_TOL, (i, np.abs(lh - lo).max())
        mean_diff.append(np.abs(lh - lo).mean())
        if nxt_h == nxt_o:
            exact += 1
        else:
            assert lo.max() - lo[nxt_h] <= LOGIT_TOL, (i, nxt_h, nxt_o, lo.max() - lo[nxt_h])
        tok = nxt_h
    assert exact >= n_gen - 5, exact
    assert np.mean(mean_diff) <= 5e-3
    # and the free-running greedy loops agree too when no near-tie is hit (seed chosen accordingly)
    res = hm.session(160).generate(prompt, prompt.size + 31)
    want, _, _ = om.session().generate(prompt, 32)
    agree = int((res["tokens"] == want).cumprod().sum())
    assert agree >= 8, (agree, res["tokens"], want)
    assert res["tokens_generated"] == 31


def test_decode_paths_agree(gpu, oracle):
    """decode_step (host loop, one sync per token), decode_n (hipGraph replay chained on device) and the un-graphed
    launch path must produce identical ids and logits -- same kernels, same order."""
    import os
    from jlama_amd import synthetic as S
    cfg = dict(S.TINY)
    hm, om, _ = _pair(cfg, 2, oracle)
    prompt = S.prompt_tokens(cfg, n=20, seed=2)
    n = 60
    s1 = hm.session(128)
    s1.batch_forward(prompt, 0)
    first = s1.sample()
    a = s1.decode_n(first, prompt.size, n)
    la = s1.logits()
    s2 = hm.session(128)
    s2.batch_forward(prompt, 0)
    assert s2.sample() == first
    b, tok = [], first
    for i in range(n):
        tok = s2.decode_step(tok, prompt.size + i)
        b.append(tok)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(la, s2.logits())
    _N.set_option("JH_NO_GRAPH", "1")
    try:
        s3 = hm.session(128)
        s3.batch_forward(prompt, 0)
        s3.sample()
        c = s3.decode_n(first, prompt.size, n)
    finally:
        _N.clear_options()
    np.testing.assert_array_equal(a, c)
    ms, k = s1.decode_stats()
    assert ms > 0 and k == cfg["n_layers"] * 5 + 2


def test_attention_split_combine_long_context(gpu, oracle):
    """Context long enough that the decode attention runs many slices (and chunk > 32): the last-arriver combine must
    match the un-split computation; also check across env-selected split counts."""
    import os
    from jlama_amd import synthetic as S
    cfg = dict(S.TINY)
    cfg["context_length"] = 2048
    hm, om, _ = _pair(cfg, 3, oracle)
    prompt = S.prompt_tokens(cfg, n=1300, seed=9)
    os_ = om.session()
    want = os_.forward(prompt, 0)[-1]
    outs = []
    for splits in ("1", "4", "16"):
        _N.set_option("JH_ATTN_SPLITS", splits)
        try:
            hs = hm.session(1400)
            got = hs.batch_forward(prompt, 0)[-1]
        finally:
            _N.clear_options()
        assert _rel(got, want) <= TRUNK_TOL, (splits, _rel(got, want))
        outs.append(got)
    assert _rel(outs[0], outs[2]) <= TRUNK_TOL


def test_out_of_range_token_is_rejected(gpu):
    from jlama_amd import _native as N, synthetic as S
    from jlama_amd.model import HipLlamaModel
    cfg = dict(S.TINY)
    hs = HipLlamaModel(cfg, S.make_weights(cfg, seed=0)).session(16)
    with pytest.raises(N.JhError):
        hs.forward([cfg["vocab_size"]], 0)
    with pytest.raises(N.JhError):
        hs.forward([3], 16)  # beyond the session's max_ctx


def test_sampling_with_temperature_uses_callers_uniform(gpu, oracle):
    from jlama_amd import synthetic as S
    cfg = dict(S.TINY)
    hm, om, _ = _pair(cfg, 4, oracle)
    prompt = S.prompt_tokens(cfg, n=6, seed=1)
    hs = hm.session(32)
    out = hs.batch_forward(prompt, 0)
    for u in (0.01, 0.3, 0.77, 0.999):
        th = hs.sample(0.8, u)
        to, _ = om.sample(out[-1], 0.8, u)
        # the oracle samples from ITS logits; equal unless u falls within the logit noise of a CDF edge
        assert th == to, (u, th, to)


def test_layer_sharded_loopback_is_bit_identical(gpu, oracle):
    """DistributedContext layer split (DistributedContext.java:75-77) with all shards on one device: shard k feeds its
    [B,E] output to shard k+1 (the PassRecord tensor, Worker.java:193-196).  Same kernels, same order => identical bits."""
    from jlama_amd import synthetic as S
    from jlama_amd.model import HipLlamaModel
    cfg = dict(S.SMALL)
    cfg["n_layers"] = 4
    w = S.make_weights(cfg, seed=6)
    full = HipLlamaModel(cfg, w)
    prompt = S.prompt_tokens(cfg, n=17, seed=4)
    ref = full.session(64).batch_forward(prompt, 0)
    for nshard in (2, 4):
        per = cfg["n_layers"] // nshard
        x = None
        for k in range(nshard):
            m = HipLlamaModel(cfg, w, layer_range=(k * per, (k + 1) * per))
            s = m.session(64)
            x = s.forward(tokens=prompt if k == 0 else None, start_pos=0, x=x)
        np.testing.assert_array_equal(x, ref)


@pytest.mark.parametrize("name", ["LLAMA32_1B", "LLAMA3_8B", "LLAMA3_70B"])
def test_real_shapes_one_layer(gpu, oracle, name):
    """BASELINE.json configs[1]/[2] shapes (E, H, heads, head size, vocab) on a 1-layer slice with a reduced vocab:
    exercises the exact kernel instantiations the bench uses (NB=1/2/7 blocks per lane, head size 64/128)."""
    from jlama_amd import synthetic as S
    cfg = dict(getattr(S, name))
    cfg.update(n_layers=1, vocab_size=2048, context_length=512, bos_token=1)
    cfg.pop("tied", None)
    hm, om, _ = _pair(cfg, 7, oracle)
    prompt = S.prompt_tokens(cfg, n=40, seed=8)
    hs, os_ = hm.session(128), om.session()
    got, want = hs.batch_forward(prompt, 0), os_.forward(prompt, 0)
    assert _rel(got, want) <= TRUNK_TOL
    th, lh = hs.sample(0.0, 0.5, want_logits=True)
    to, lo = om.sample(want[-1])
    assert np.abs(lh - lo).max() <= LOGIT_TOL
    assert th == to or lo.max() - lo[th] <= LOGIT_TOL
    # teacher-forced decode through the hipGraph path: ids equal wherever the oracle's margin is meaningful
    got_tokens = hs.decode_n(th, prompt.size, 24)
    tok = th
    for i, g in enumerate(got_tokens):
        xo = os_.forward([tok], prompt.size + i)
        no, lo = om.sample(xo[-1])
        assert g == no or lo.max() - lo[g] <= LOGIT_TOL, (i, g, no)
        tok = int(g)


@pytest.mark.parametrize("cfgname", ["TINY", "SMALL"])
def test_bf16_model_parity(gpu, oracle, cfgname):
    """BF16 dense model (config 4 family: BF16 weights, BF16-rounded activations, F32 accumulate, F32xBF16 LM head):
    layer-0 taps, teacher-forced logits and greedy ids vs the oracle's GemmerBF16 / GemmerF32BF16 restatement."""
    from jlama_amd import _native as N, synthetic as S
    cfg = dict(getattr(S, cfgname))
    cfg["weight_dtype"] = N.DT_BF16
    hm, om, _ = _pair(cfg, 5, oracle)
    prompt = S.prompt_tokens(cfg, n=37, seed=6)
    E, A = cfg["embedding_length"], cfg["n_heads"] * cfg["head_size"]
    hs2, os2 = hm.session(64), om.session()
    hs2.set_tap_layer(0)
    os2.set_tap_layer(0)
    hs2.forward([prompt[0]], 0, want_output=False)
    os2.forward([prompt[0]], 0)
    for name, n in [("input_emb", E), ("query", A), ("after_attention", A), ("post_ff_res", E)]:
        assert _rel(hs2.tap(name, n), os2.tap(name, n)) <= 1e-4, name
    hs, os_ = hm.session(96), om.session()
    out_h, out_o = hs.batch_forward(prompt, 0), os_.forward(prompt, 0)
    assert _rel(out_h, out_o) <= TRUNK_TOL
    tok, lh = hs.sample(0.0, 0.5, want_logits=True)
    tok_o, lo = om.sample(out_o[-1])
    assert np.abs(lh - lo).max() <= LOGIT_TOL
    assert tok == tok_o or lo.max() - lo[tok] <= LOGIT_TOL
    got = hs.decode_n(tok, prompt.size, 32)
    for i, g in enumerate(got):
        xo = os_.forward([tok], prompt.size + i)
        no, lo = om.sample(xo[-1])
        assert g == no or lo.max() - lo[g] <= LOGIT_TOL, (i, g, no)
        tok = int(g)


def test_bf16_mistral_shapes_one_layer(gpu, oracle):
    from jlama_amd import synthetic as S
    cfg = dict(S.MISTRAL_7B)
    cfg.update(n_layers=1, vocab_size=2048, context_length=512)
    hm, om, _ = _pair(cfg, 8, oracle)
    prompt = S.prompt_tokens(cfg, n=12, seed=3)
    got, want = hm.session(64).batch_forward(prompt, 0), om.session().forward(prompt, 0)
    assert _rel(got, want) <= TRUNK_TOL


@pytest.mark.parametrize("dtype", ["Q4", "BF16"])
def test_batched_prefill_matches_row_path_and_oracle(gpu, oracle, monkeypatch, dtype):
    """batchForward (AbstractModel.java:295-312): prompt chunks of up to 256 rows run as MFMA GEMMs over all rows +
    causal attention per row; the result must agree with the one-position-at-a-time path (batchForwardSlow order,
    :282-290) and with the oracle, including a 300-row prompt (two chunks) and a continuation at start_pos > 0, and
    must leave the KV pages / current row in the state the decode path expects."""
    from jlama_amd import _native as N, synthetic as S
    cfg = dict(S.SMALL)
    if dtype == "BF16":
        cfg["weight_dtype"] = N.DT_BF16   # BF16 x BF16 MFMA GEMMs, activations RNE-rounded per row
    hm, om, _ = _pair(cfg, 21, oracle)
    prompt = S.prompt_tokens(cfg, n=300, seed=22)
    want = om.session().forward(prompt, 0)
    _N.set_option("JH_PREFILL_BATCH_MIN", "0")
    s_row = hm.session(512)
    rows = s_row.forward(prompt, 0)
    _N.clear_options()
    s_bat = hm.session(512)
    bat = s_bat.forward(prompt, 0)
    assert bat.shape == rows.shape == want.shape
    assert _rel(bat, want) <= TRUNK_TOL and _rel(rows, want) <= TRUNK_TOL
    assert _rel(bat, rows) <= TRUNK_TOL
    if dtype == "Q4":   # short contexts, before any I8 code flips: float-ordering noise only (BF16 rounding flips at once)
        assert np.abs(bat - rows)[:4].max() <= 1e-5
    # split call: [0,100) then [100,300) at start_pos=100 (chunked prefill against existing KV pages)
    s_two = hm.session(512)
    a = s_two.forward(prompt[:100], 0)
    b = s_two.forward(prompt[100:], 100)
    assert _rel(np.concatenate([a, b]), want) <= TRUNK_TOL
    # sampling + graph decode continue from the batched prefill's state
    ob = om.session()
    ob.forward(prompt, 0)
    for s in (s_bat, s_two):
        th, lh = s.sample(0.0, 0.5, want_logits=True)
        to, lo = om.sample(want[-1])
        assert np.abs(lh - lo).max() <= LOGIT_TOL
        assert th == to or lo.max() - lo[th] <= LOGIT_TOL
    got = s_bat.decode_n(th, prompt.size, 12)
    tok = th
    for i, g in enumerate(got):
        xo = ob.forward([tok], prompt.size + i)
        no, lo = om.sample(xo[-1])
        assert g == no or lo.max() - lo[g] <= LOGIT_TOL, (i, g, no)
        tok = int(g)


@pytest.mark.parametrize("dtype", ["Q4", "BF16"])
def test_prefill_without_a_resident_second_copy_of_the_weights(gpu, oracle, monkeypatch, dtype):
    """JH_TILED_COPY=transient: the MFMA-ordered operand of every prefill GEMM is rebuilt in a per-session scratch in front
    of the GEMM instead of living in HBM as a second copy of the model.  Same kernels, same operand bytes: the rows must be
    bit-identical to the resident mode's, across two chunks (the scratch is reused by every GEMM of every layer and by the
    replayed prefill graph), and the model must report no tiled bytes."""
    from jlama_amd import _native as N, synthetic as S
    cfg = dict(S.SMALL)
    if dtype == "BF16":
        cfg["weight_dtype"] = N.DT_BF16
    prompt = S.prompt_tokens(cfg, n=300, seed=22)
    _N.set_option("JH_TILED_COPY", "resident")
    hm, om, _ = _pair(cfg, 21, oracle)
    s1 = hm.session(512)
    res = s1.forward(prompt, 0)
    assert hm.tiled_bytes() > 0.8 * sum(r * c for r, c in S.layer_shapes(cfg).values()) * cfg["n_layers"] * (0.625 if dtype == "Q4" else 2.0)
    _N.set_option("JH_TILED_COPY", "transient")
    hm2, _, _ = _pair(cfg, 21, oracle)
    s2 = hm2.session(512)
    tra = s2.forward(prompt, 0)
    again = hm2.session(512).forward(prompt, 0)
    assert hm2.tiled_bytes() == 0
    assert np.array_equal(tra, res) and np.array_equal(again, res)
    assert _rel(tra, om.session().forward(prompt, 0)) <= TRUNK_TOL
    t1, l1 = s1.sample(0.0, 0.5, want_logits=True)
    t2, l2 = s2.sample(0.0, 0.5, want_logits=True)
    assert t1 == t2 and np.array_equal(l1, l2)
    assert list(s1.decode_n(t1, prompt.size, 8)) == list(s2.decode_n(t2, prompt.size, 8))


@pytest.mark.parametrize("shards", [1, 2])
def test_checkpoint_loads_straight_into_hbm(gpu, oracle, tmp_path, shards):
    """f1: a JQ4 safetensors checkpoint directory (config.json + model.safetensors[.index.json]) -> resident model via
    the mmap'd bytes; identical bits to the model built from the in-memory tensors, and oracle parity on top."""
    from jlama_amd import safetensors_jq4 as ST, synthetic as S
    from jlama_amd.model import HipLlamaModel
    cfg = dict(S.SMALL)
    w = S.make_weights(cfg, seed=31)
    d = str(tmp_path / "ckpt")
    ST.write_llama_checkpoint(d, cfg, w, shards=shards)
    prompt = S.prompt_tokens(cfg, n=20, seed=9)
    ref = HipLlamaModel(cfg, w)
    got = ST.load_llama(d)
    assert got.weight_bytes() == ref.weight_bytes()
    sr, sg = ref.session(64), got.session(64)
    np.testing.assert_array_equal(sg.forward(prompt, 0), sr.forward(prompt, 0))
    tr, lr = sr.sample(0.0, 0.5, want_logits=True)
    tg, lg = sg.sample(0.0, 0.5, want_logits=True)
    assert tr == tg
    np.testing.assert_array_equal(lg, lr)
    np.testing.assert_array_equal(sg.decode_n(tg, prompt.size, 8), sr.decode_n(tr, prompt.size, 8))
    # layer shards read only their own tensors and chain to the same result
    x = None
    for k, rng in enumerate(((0, 1), (1, 3))):
        m = ST.load_llama(d, layer_range=rng)
        x = m.session(64).forward(tokens=prompt if k == 0 else None, start_pos=0, x=x)
    np.testing.assert_array_equal(x, ref.session(64).forward(prompt, 0))
    om = oracle.OracleModel(cfg, w)
    assert _rel(x, om.session().forward(prompt, 0)) <= TRUNK_TOL


@pytest.mark.parametrize("dtype", ["Q4", "BF16"])
def test_tensor_parallel_shards_loopback(gpu, oracle, dtype):
    """f2: two head-split shards (local heads / kv heads / hidden rows, o/down K windows, global RoPE head index) resident
    on ONE device, the all-reduce replaced by an in-order sum of the two partial vectors: must agree with the oracle's
    lock-step shard restatement (jo_forward_tp) and sit within the Q8 noise floor of the un-sharded model."""
    import torch
    from jlama_amd import _native as N, distributed as D, synthetic as S
    from jlama_amd.model import HipLlamaModel
    cfg = dict(S.SMALL)
    if dtype == "BF16":
        cfg["weight_dtype"] = N.DT_BF16
    w = S.make_weights(cfg, seed=41)
    prompt = S.prompt_tokens(cfg, n=12, seed=7)
    size, E, L = 2, cfg["embedding_length"], cfg["n_layers"]
    shards, osess = [], []
    for r in range(size):
        lc, off = D.tp_shard_config(cfg, r, size)
        sw = D.tp_shard_weights(cfg, w, r, size)
        shards.append(HipLlamaModel(lc, sw, kv_head_offset=off).session(64))
        osess.append(oracle.OracleModel(lc, sw, kv_head_offset=off).session())
    dev = torch.device("cuda", 0)
    part = [torch.empty(E, dtype=torch.float32, device=dev) for _ in range(size)]
    rows = []
    for pos, tok in enumerate(prompt):
        for s in shards:
            s.tp_set_row(int(tok), pos)
        for li in range(L):
            for s, p in zip(shards, part):
                s.tp_attn(li, p.data_ptr())
                s.synchronize()
            red = part[0] + part[1]
            torch.cuda.synchronize()
            for s, p in zip(shards, part):
                s.tp_ffn(li, red.data_ptr(), p.data_ptr())
                s.synchronize()
            red2 = part[0] + part[1]
            torch.cuda.synchronize()
            for s in shards:
                s.tp_finish_layer(red2.data_ptr())
                s.synchronize()
        rows.append(shards[0].current_row())
        np.testing.assert_array_equal(rows[-1], shards[1].current_row())     # every shard holds the same residual stream
    got = np.stack(rows)
    want_tp = oracle.forward_tp(osess, prompt, 0)
    assert _rel(got, want_tp) <= TRUNK_TOL
    assert np.abs(got[0] - want_tp[0]).max() <= (1e-4 if dtype == "Q4" else 3e-2) * np.abs(want_tp[0]).max()
    full = oracle.OracleModel(cfg, w)
    assert _rel(got, full.session().forward(prompt, 0)) <= TRUNK_TOL


@pytest.mark.parametrize("cfgname", ["TINY", "SMALL"])
def test_decode_across_attention_variants_and_long_context(gpu, oracle, cfgname):
    """The decode attention kernel has a short-context variant (2 prefetched row steps, contexts <= 16*32 rows) and the
    general one; the host switches graphs per token.  Greedy decode from position ~500 to ~530 crosses the switch, and a
    second run decodes at ~1300 rows where slices are longer than the prefetched rows (tail loops): teacher-forced
    against the oracle, ids equal wherever the oracle's margin is meaningful."""
    from jlama_amd import synthetic as S
    cfg = dict(getattr(S, cfgname))
    cfg["context_length"] = 2048
    hm, om, _ = _pair(cfg, 13, oracle)
    for n_prompt, n_dec in ((499, 30), (1290, 10)):
        prompt = S.prompt_tokens(cfg, n=n_prompt, seed=17)
        hs, os_ = hm.session(n_prompt + n_dec + 8), om.session()
        got, want = hs.batch_forward(prompt, 0), os_.forward(prompt, 0)
        assert _rel(got[-1], want[-1]) <= TRUNK_TOL
        th, lh = hs.sample(0.0, 0.5, want_logits=True)
        to, lo = om.sample(want[-1])
        assert th == to or lo.max() - lo[th] <= LOGIT_TOL
        toks = hs.decode_n(th, prompt.size, n_dec)
        tok = th
        for i, g in enumerate(toks):
            xo = os_.forward([tok], prompt.size + i)
            no, lo = om.sample(xo[-1])
            assert g == no or lo.max() - lo[g] <= LOGIT_TOL, (n_prompt, i, g, no)
            tok = int(g)
        # the same positions through the host loop (jh_forward row graph + jh_sample) give the same ids
        hs2 = hm.session(n_prompt + n_dec + 8)
        hs2.batch_forward(prompt, 0)
        tok2 = hs2.sample(0.0, 0.5)
        assert tok2 == th
        for i in range(min(6, n_dec)):
            tok2 = hs2.decode_step(tok2, prompt.size + i)
            assert tok2 == toks[i], (n_prompt, i)


def test_replacing_a_weight_invalidates_captured_graphs(gpu, oracle):
    """Captured decode / prefill graphs and the MFMA-ordered weight copies hold device pointers: after
    jh_model_set_weight on a live model the session must re-capture and re-tile, and match a model built from the new
    weights from scratch."""
    from jlama_amd import synthetic as S
    from jlama_amd.model import HipLlamaModel
    cfg = dict(S.SMALL)
    w_a, w_b = S.make_weights(cfg, seed=51), S.make_weights(cfg, seed=52)
    prompt = S.prompt_tokens(cfg, n=40, seed=3)
    m = HipLlamaModel(cfg, w_a)
    s = m.session(96)
    s.batch_forward(prompt, 0)
    t = s.sample(0.0, 0.5)
    s.decode_n(t, prompt.size, 4)                       # graphs of every kind now exist for the old weights
    for key in ((1, S.W_GATE), (1, S.W_UP), (0, S.W_Q), (2, S.W_DOWN)):
        m.set_weight(key[0], key[1], w_b[key])
    w_mix = dict(w_a)
    for key in ((1, S.W_GATE), (1, S.W_UP), (0, S.W_Q), (2, S.W_DOWN)):
        w_mix[key] = w_b[key]
    ref = HipLlamaModel(cfg, w_mix).session(96)
    np.testing.assert_array_equal(s.forward(prompt, 0), ref.forward(prompt, 0))
    ta, tb = s.sample(0.0, 0.5), ref.sample(0.0, 0.5)
    assert ta == tb
    np.testing.assert_array_equal(s.decode_n(ta, prompt.size, 6), ref.decode_n(tb, prompt.size, 6))


def test_decode_attention_long_slices(gpu, oracle):
    """Decode where a slice of the context holds more rows than the kernel prefetches (128 for head size 128), so the
    batched tail rounds of the score and PV loops run: a 700-row context cut into 4 slices (175 rows) and 2 slices
    (350 rows) via JH_ATTN_SPLITS.  Teacher-forced vs the oracle."""
    import os
    from jlama_amd import synthetic as S
    cfg = dict(S.SMALL)
    cfg["context_length"] = 1024
    hm, om, _ = _pair(cfg, 19, oracle)
    prompt = S.prompt_tokens(cfg, n=699, seed=23)
    os_ = om.session()
    want = os_.forward(prompt, 0)
    first, lo = om.sample(want[-1])
    ref_toks, ref_margin, tok = [], [], first
    for i in range(5):
        xo = os_.forward([tok], prompt.size + i)
        tok, lg = om.sample(xo[-1])
        top2 = np.partition(lg, -2)[-2:]
        ref_toks.append(tok)
        ref_margin.append(float(top2[1] - top2[0]))
    for splits in ("4", "2"):
        _N.set_option("JH_ATTN_SPLITS", splits)
        try:
            hs = hm.session(800)
            got = hs.batch_forward(prompt, 0)
            assert _rel(got[-1], want[-1]) <= TRUNK_TOL
            t0, lh = hs.sample(0.0, 0.5, want_logits=True)
            assert np.abs(lh - lo).max() <= LOGIT_TOL
            toks = [first]   # teacher-forced: feed the oracle's tokens, compare each sampled id
            for i in range(5):
                g = hs.decode_step(toks[-1], prompt.size + i)
                assert g == ref_toks[i] or ref_margin[i] <= LOGIT_TOL, (splits, i, g, ref_toks[i])
                toks.append(ref_toks[i])
        finally:
            _N.clear_options()


@pytest.mark.parametrize("rows", [129, 37, 264])
def test_prefill_ragged_last_row_tile(gpu, oracle, monkeypatch, rows):
    """Prompts whose last 32-row tile is nearly empty (the metric's 129 = 4*32 + 1; 37; 264): rows past M are computed on
    replicated / clamped operands and never stored.  Batched prefill (default dispatch and each I8xQ4 GEMM kernel forced)
    against the one-position-at-a-time path and the oracle, single layer so that a tipped Q8 code stays in its row."""
    from jlama_amd import synthetic as S
    cfg = dict(S.SMALL)
    cfg["embedding_length"], cfg["hidden_length"], cfg["n_layers"] = 1024, 2048, 1
    hm, om, _ = _pair(cfg, 37, oracle)
    prompt = S.prompt_tokens(cfg, n=rows, seed=38)
    want = om.session().forward(prompt, 0)
    _N.set_option("JH_PREFILL_BATCH_MIN", "0")
    row = hm.session(512).forward(prompt, 0)
    _N.clear_options()
    got = [hm.session(512).forward(prompt, 0)]
    _N.set_option("JH_GEMM_LDS", "1")
    got.append(hm.session(512).forward(prompt, 0))
    _N.set_option("JH_GEMM_LDS", "0")
    got.append(hm.session(512).forward(prompt, 0))
    for g in got:
        assert g.shape == want.shape and _rel(g, want) <= TRUNK_TOL and _rel(g, row) <= TRUNK_TOL
        per_row = np.abs(g - row).max(axis=1)
        assert np.mean(per_row <= 1e-5) >= 0.8 and per_row[-1] <= FLIP_ROW, (np.sort(per_row)[-6:], per_row[-1])


def test_decode_attention_slice_tiers(gpu, oracle, monkeypatch):
    """The decode-attention kernel is captured in three variants chosen by the host from the position it already knows: short
    contexts (slices of <= 32 rows, 2 prefetched row steps), medium, and long contexts with more slices (up to mid_splits up to
    mid_max rows, long_splits beyond).  With the thresholds pulled down to a toy context every tier and every boundary is
    crossed, by the single-row graph (forward + sample) and by the device-resident loop (decode_n): logits equal the default
    configuration's to float-ordering noise (the slicing only changes where partial softmax sums are merged)."""
    from jlama_amd import synthetic as S
    cfg = dict(S.SMALL)
    hm, om, _ = _pair(cfg, 31, oracle)
    prompt = S.prompt_tokens(cfg, n=40, seed=33)
    base = hm.session(256)
    base.batch_forward(prompt, 0)
    for k, v in (("JH_ATTN_SPLITS", "2"), ("JH_ATTN_LONG_MIN", "100"), ("JH_ATTN_LONG_SPLITS", "8"), ("JH_ATTN_MID_SPLITS", "4"),
                 ("JH_ATTN_MID_MAX", "150")):
        _N.set_option(k, v)
    tier = hm.session(256)          # variant 1 up to 64 rows, 0 up to 100, 2 beyond: <= 4 slices up to 150 rows, <= 8 after
    tier2 = hm.session(256)
    for k in ("JH_ATTN_SPLITS", "JH_ATTN_LONG_MIN", "JH_ATTN_LONG_SPLITS", "JH_ATTN_MID_SPLITS", "JH_ATTN_MID_MAX"):
        _N.clear_options()
    tier.batch_forward(prompt, 0)
    tier2.batch_forward(prompt, 0)
    tb, lb = base.sample(0.0, 0.5, want_logits=True)
    tt, lt = tier.sample(0.0, 0.5, want_logits=True)
    assert tb == tt and np.abs(lb - lt).max() <= 1e-4
    toks, dev = [tb], []
    for i in range(140):            # positions 40 .. 179, teacher-forced with the default session's ids
        pos = prompt.size + i
        base.forward([toks[-1]], pos, want_output=False)
        tier.forward([toks[-1]], pos, want_output=False)
        tb, lb = base.sample(0.0, 0.5, want_logits=True)
        tt, lt = tier.sample(0.0, 0.5, want_logits=True)
        dev.append(float(np.abs(lb - lt).max()))
        top2 = np.partition(lb, -2)[-2:]
        assert tt == tb or top2[1] - top2[0] <= LOGIT_TOL, (pos, tt, tb)
        toks.append(tb)
    # merge-order noise is 1e-6; now and then it tips a Q8 code downstream (one code step ~1e-2 of a row) and that row's K/V stay
    # in the cache for the rest of the run: every step stays inside the flip envelope (a mis-merged slice would be O(1) off),
    # and up to the first tipped code the logits agree to noise
    assert max(dev) <= LOGIT_TOL, max(dev)
    clean = next((i for i, d in enumerate(dev) if d > 1e-4), len(dev))
    assert clean >= 26 and max(dev[:clean] + [0.0]) <= 1e-5, (clean, dev[:40])   # 24 steps share the slicing; the tiers differ after
    got = np.asarray(tier2.decode_n(toks[0], prompt.size, 140))     # the captured decode loop walks through the same tiers
    same = got == np.asarray(toks[1:])
    first_diff = int(np.argmin(same)) if not same.all() else same.size
    assert first_diff >= 60, first_diff   # free-running: identical until a near-tie, far beyond the first two tier boundaries


@pytest.mark.parametrize("shape", ["4,1,2", "2,1,4", "4,1,1", "4,2,2"])
def test_prefill_gemm_lds_kernel_equals_tile_kernel(gpu, oracle, monkeypatch, shape):
    """gemm_q8q4_lds_kernel (A through LDS, K split over the waves of a workgroup; the default for gate|up and down at model
    size) against gemm_q8q4_tile_kernel on the same 300-row prompt: the integer block sums are exact in both and the per-block
    scaling is the same expression, so rows agree to float-ordering noise where the K split differs (bar the rare Q8 code
    that the noise tips over its rounding edge) and the batched prefill keeps its distance to the oracle.  JH_GEMM_Z = 2 adds the cross-workgroup K split (workspace + splitk_reduce_kernel)."""
    from jlama_amd import synthetic as S
    cfg = dict(S.SMALL)
    # 32 / 64 Q blocks per row: every K split divides.  ONE layer: a tipped Q8 code then stays in its own row (with more layers
    # it reaches every later row through the K/V it changes)
    cfg["embedding_length"], cfg["hidden_length"], cfg["n_layers"] = 1024, 2048, 1
    hm, om, _ = _pair(cfg, 27, oracle)
    prompt = S.prompt_tokens(cfg, n=300, seed=28)
    want = om.session().forward(prompt, 0)
    _N.set_option("JH_GEMM_LDS", "0")
    tile = hm.session(512).forward(prompt, 0)
    cw, ct, sk = shape.split(",")
    _N.set_option("JH_GEMM_LDS", "1")
    _N.set_option("JH_GEMM_LDS_CW", cw)
    _N.set_option("JH_GEMM_LDS_CT", ct)
    _N.set_option("JH_GEMM_LDS_S", sk)
    lds = hm.session(512).forward(prompt, 0)
    _N.set_option("JH_GEMM_Z", "2")
    ldz = hm.session(512).forward(prompt, 0)
    for got in (lds, ldz):
        assert _rel(got, want) <= TRUNK_TOL and _rel(got, tile) <= TRUNK_TOL
        # summation-order noise only (1e-7) unless it tips a Q8 code of a later quantization over its rounding edge: such rows
        # differ by one code step (1e-2 of the row scale); they are a small minority
        per_row = np.abs(got - tile).max(axis=1)
        assert np.mean(per_row <= 1e-5) >= 0.8, np.sort(per_row)[-8:]


@pytest.mark.parametrize("cfgname,mfma_min", [("SMALL", "0"), ("TINY", "0"), ("SMALL", "100")])
def test_blockwise_mfma_prefill_attention(gpu, oracle, monkeypatch, cfgname, mfma_min):
    """f4: attn_prefill_mfma_kernel (32-row query tiles x K/V tiles on v_mfma_f32_32x32x2_f32, online softmax, key-range
    splits + combine) against the one-position-at-a-time decode path and the oracle: a 300-row prompt in two chunks (the
    second starts at position 256: query tiles not aligned with... key tiles are absolute), a continuation at an odd
    start position, head sizes 128 (SMALL, 4 heads per kv head) and 64 (TINY, 2 per kv head)."""
    from jlama_amd import synthetic as S
    cfg = dict(getattr(S, cfgname))
    cfg["context_length"] = 1024
    hm, om, _ = _pair(cfg, 23, oracle)
    prompt = S.prompt_tokens(cfg, n=300, seed=24)
    want = om.session().forward(prompt, 0)
    _N.set_option("JH_PREFILL_BATCH_MIN", "0")
    rows = hm.session(512).forward(prompt, 0)                 # decode kernels, one position at a time
    _N.clear_options()
    _N.set_option("JH_PREFILL_ATTN_MFMA_MIN", mfma_min)
    s = hm.session(512)
    bat = s.forward(prompt, 0)
    assert _rel(bat, want) <= TRUNK_TOL and _rel(bat, rows) <= TRUNK_TOL
    # float-ordering noise only, except where an I8 code flipped downstream (rare in the first rows: short contexts)
    early = np.abs(bat - rows)[:8].max(axis=1) / np.abs(rows)[:8].max(axis=1)
    assert np.median(early) <= 1e-5 and early.min() <= 1e-6, early
    # odd split: [0,37) then [37,300): the second call's query tiles start at position 37, key tiles at multiples of 32
    s2 = hm.session(512)
    a = s2.forward(prompt[:37], 0)
    b = s2.forward(prompt[37:], 37)
    assert _rel(np.concatenate([a, b]), want) <= TRUNK_TOL
    # the KV pages / current row are what the decode path expects
    th, lh = s.sample(0.0, 0.5, want_logits=True)
    to, lo = om.sample(want[-1])
    assert np.abs(lh - lo).max() <= LOGIT_TOL
    ob = om.session()
    ob.forward(prompt, 0)
    tok = th
    for i, g in enumerate(s.decode_n(th, prompt.size, 8)):
        xo = ob.forward([tok], prompt.size + i)
        no, lo = om.sample(xo[-1])
        assert g == no or lo.max() - lo[g] <= LOGIT_TOL, (i, g, no)
        tok = int(g)


def test_blockwise_prefill_attention_is_exact_in_isolation(gpu, oracle, monkeypatch):
    """The attention block alone, one layer, no quantizer downstream of it in the comparison: the `after_attention`
    rows of the MFMA kernel against the per-row kernel on IDENTICAL q/k/v (same session weights, same prompt) must agree
    to float-ordering level (1e-5 of the row scale) for every row of a 700-row prompt (3 chunks, key-range splits)."""
    from jlama_amd import synthetic as S
    cfg = dict(S.SMALL)
    cfg.update(n_layers=1, context_length=1024)
    hm, om, _ = _pair(cfg, 29, oracle)
    prompt = S.prompt_tokens(cfg, n=699, seed=30)
    _N.set_option("JH_PREFILL_ATTN_MFMA_MIN", "-1")
    ref = hm.session(800).forward(prompt, 0)
    _N.set_option("JH_PREFILL_ATTN_MFMA_MIN", "0")
    got = hm.session(800).forward(prompt, 0)
    # one layer: the outputs differ only through the attention rows (then one Q8 step); most rows see no code flip
    rel = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
    assert rel.max() <= 1.5e-2 and np.median(rel) <= 1e-5, (rel.max(), np.median(rel))
    want = om.session().forward(prompt, 0)
    assert _rel(got, want) <= TRUNK_TOL


@pytest.mark.parametrize("stages", [2, 4])
def test_one_process_pipeline_loopback_is_bit_identical(gpu, oracle, stages):
    """jh_pipeline_*: the one-process layer-sharded host (BASELINE north_star) with every stage on device 0 -- peer copies
    degenerate to device-to-device copies, the event choreography, per-stage position words, token feedback and hop-buffer
    reuse are the multi-GPU ones.  Prompt longer than one 256-row chunk, then 40 greedy steps crossing the attention-variant
    switch: ids and logits identical to the un-sharded model (same kernels, same order)."""
    from jlama_amd import synthetic as S
    from jlama_amd.model import HipLlamaModel, HipPipeline, build_stage_models
    cfg = dict(S.SMALL)
    cfg.update(n_layers=4, context_length=1024)
    w = S.make_weights(cfg, seed=6, quantize=oracle.q4_quantize)
    prompt = S.prompt_tokens(cfg, n=299, seed=4)
    full = HipLlamaModel(cfg, w).session(600)
    full.batch_forward(prompt, 0)
    first = full.sample()
    want = full.decode_n(first, prompt.size, 240)
    models = build_stage_models(cfg, lambda k, rng, dev: w, [0] * stages)
    pipe = HipPipeline(models, 600)
    assert pipe.prefill(prompt) == first
    got = pipe.decode_n(first, prompt.size, 240)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(pipe.sessions[-1].logits(), full.logits())
    # a second prompt on the same pipeline (hop buffers and events are reused)
    p2 = S.prompt_tokens(cfg, n=40, seed=5)
    full2 = HipLlamaModel(cfg, w).session(600)
    full2.batch_forward(p2, 0)
    f2 = full2.sample()
    assert pipe.prefill(p2) == f2
    np.testing.assert_array_equal(pipe.decode_n(f2, p2.size, 16), full2.decode_n(f2, p2.size, 16))
    # two pipelines over the same stage models, both queued before either is awaited (two sessions in flight)
    pa, pb = HipPipeline(models, 600), HipPipeline(models, 600)
    fa, fb = pa.prefill(prompt), pb.prefill(p2)
    pa.decode_n_async(fa, prompt.size, 32)
    pb.decode_n_async(fb, p2.size, 32)
    np.testing.assert_array_equal(pa.decode_wait(32), want[:32])
    np.testing.assert_array_equal(pb.decode_wait(32), full2.decode_n(f2, p2.size, 32))
    for q in (pipe, pa, pb):
        q.close()


class _LoopbackDist:
    """torch.distributed's send / recv / isend / broadcast between THREADS of one process (one per pipeline rank), so the
    rank-per-GPU pipeline code (jlama_amd.distributed.pipeline_prefill / pipeline_decode + HipShardEngine) can run with
    every shard on the one GPU of the test box.  Messages are device tensors cloned at send time."""

    def __init__(self, rank, world, queues, torch, lock):
        self.rank, self.world, self.q, self.torch, self.lock = rank, world, queues, torch, lock

    class _Done:
        def wait(self):
            return None

    def send(self, t, dst):
        with self.lock:
            self.torch.cuda.synchronize()
            c = t.clone()
            self.torch.cuda.synchronize()
        self.q[(self.rank, dst)].put(c)

    def isend(self, t, dst):
        self.send(t, dst)
        return self._Done()

    def recv(self, t, src):
        m = self.q[(src, self.rank)].get(timeout=120)
        with self.lock:
            t.copy_(m)
            self.torch.cuda.synchronize()

    def broadcast(self, t, src):
        if self.rank == src:
            for d in range(self.world):
                if d != src:
                    self.send(t, d)
        else:
            self.recv(t, src)


@pytest.mark.parametrize("world", [2, 4])
def test_rank_per_gpu_pipeline_engine_loopback(gpu, oracle, world):
    """The code bench.py runs for --gpus N (HipShardEngine + pipeline_prefill / pipeline_decode) with N shards on ONE
    device and an in-process transport: N sessions in flight and the single-stream form both reproduce the un-sharded
    model's ids exactly."""
    import queue
    import threading
    import torch
    from jlama_amd import distributed as D, synthetic as S
    from jlama_amd.model import HipLlamaModel
    cfg = dict(S.SMALL)
    cfg["n_layers"] = 4
    w = S.make_weights(cfg, seed=6, quantize=oracle.q4_quantize)
    E, steps = cfg["embedding_length"], 12
    prompts = [S.prompt_tokens(cfg, n=20, seed=100 + j) for j in range(world)]
    want = []
    full = HipLlamaModel(cfg, w)
    for j in range(world):
        s = full.session(64)
        s.batch_forward(prompts[j], 0)
        f = s.sample()
        want.append((f, s.decode_n(f, prompts[j].size, steps)))
    queues = {(a, b): queue.Queue() for a in range(world) for b in range(world)}
    results, errors = {}, []
    dev = torch.device("cuda", 0)
    gpu_lock = threading.Lock()

    class LockedEngine(D.HipShardEngine):
        """In the real launch every rank is its own process; here the ranks are threads of one process sharing one HIP
        runtime, so device work of different ranks is serialised (hipGraph capture is not robust against other threads'
        runtime calls).  The transport and the pipeline schedule are unaffected."""

        def forward_tokens(self, *a):
            with gpu_lock:
                return super().forward_tokens(*a)

        def forward_x(self, *a):
            with gpu_lock:
                return super().forward_x(*a)

        def sample(self, *a):
            with gpu_lock:
                return super().sample(*a)

    def rank_main(rank):
        try:
            torch.cuda.set_device(0)
            dist = _LoopbackDist(rank, world, queues, torch, gpu_lock)
            eng = engines[rank]
            firsts = [D.pipeline_prefill(dist, eng, rank, world, j, prompts[j], E, dev, torch.float32) for j in range(world)]
            toks = D.pipeline_decode(dist, eng, rank, world, firsts, prompts[0].size, steps, E, dev, torch.float32)
            single = D.pipeline_decode(dist, eng, rank, world, firsts[:1], prompts[0].size, steps, E, dev, torch.float32, n_sessions=1)
            results[rank] = (firsts, toks, single)
        except Exception as e:   # noqa: BLE001
            import traceback
            errors.append((rank, traceback.format_exc()))

    # shard engines are built here, one after the other: device / context initialisation racing with other threads' allocations
    # is a property of threads-as-ranks (one HIP runtime), not of the rank-per-process launch
    engines = [LockedEngine(cfg, w, r, world, 0, n_sessions=world, max_ctx=64) for r in range(world)]
    torch.cuda.synchronize()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors[0][1]
    firsts, toks, single = results[world - 1]
    for j in range(world):
        assert firsts[j] == want[j][0]
        np.testing.assert_array_equal(toks[j], want[j][1])
    np.testing.assert_array_equal(single[0], want[0][1])


class _StreamLoopbackDist:
    """The stream-ordered half of torch.distributed's NCCL semantics between THREADS of one process: ``isend`` snapshots
    the tensor on the CURRENT stream and records an event; ``recv`` blocks the host only until the peer has *enqueued* its
    send, then makes the current stream wait for that event and copies -- nothing waits for the GPU.  That is how RCCL
    send/recv behave under ``torch.cuda.stream(session stream)`` in pipeline_decode_streamed."""

    def __init__(self, rank, world, queues, torch, lock):
        self.rank, self.world, self.q, self.torch, self.lock = rank, world, queues, torch, lock

    class _Done:
        def wait(self):
            return None

    def isend(self, t, dst):
        with self.lock:
            c = t.clone()
            ev = self.torch.cuda.Event()
            ev.record(self.torch.cuda.current_stream())
        self.q[(self.rank, dst)].put((c, ev))
        return self._Done()

    def recv(self, t, src):
        c, ev = self.q[(src, self.rank)].get(timeout=120)
        with self.lock:
            cur = self.torch.cuda.current_stream()
            cur.wait_event(ev)
            t.copy_(c)
            c.record_stream(cur)   # the snapshot was allocated on the sender's stream


@pytest.mark.parametrize("world", [2, 4])
def test_rank_per_gpu_pipeline_stream_ordered_loopback(gpu, oracle, world):
    """pipeline_decode_streamed + jh_stage_decode_async: the rank-per-GPU decode loop with every hop ordered on the sessions'
    own streams (token id fed back as a device word, no host synchronisation inside the loop).  N shards on ONE device,
    in-process transport with NCCL's stream semantics: ids equal the un-sharded model's, sessions in flight and single stream."""
    import queue
    import threading
    import torch
    from jlama_amd import distributed as D, synthetic as S
    from jlama_amd.model import HipLlamaModel
    cfg = dict(S.SMALL)
    cfg["n_layers"] = 4
    w = S.make_weights(cfg, seed=16, quantize=oracle.q4_quantize)
    E, steps = cfg["embedding_length"], 12
    prompts = [S.prompt_tokens(cfg, n=20, seed=300 + j) for j in range(world)]
    want = []
    full = HipLlamaModel(cfg, w)
    for j in range(world):
        s = full.session(64)
        s.batch_forward(prompts[j], 0)
        f = s.sample()
        want.append((f, s.decode_n(f, prompts[j].size, steps)))
    queues = {(a, b): queue.Queue() for a in range(world) for b in range(world)}
    results, errors = {}, []
    dev = torch.device("cuda", 0)
    gpu_lock = threading.Lock()
    ready = threading.Barrier(world)

    class LockedEngine(D.HipShardEngine):
        """Ranks are threads here (one HIP runtime): runtime calls of different ranks are serialised, the GPU work is not."""

        def forward_tokens(self, *a):
            with gpu_lock:
                return super().forward_tokens(*a)

        def forward_x(self, *a):
            with gpu_lock:
                return super().forward_x(*a)

        def sample(self, *a):
            with gpu_lock:
                return super().sample(*a)

        def stage_step(self, *a):
            with gpu_lock:
                return super().stage_step(*a)

    def rank_main(rank):
        try:
            torch.cuda.set_device(0)
            host = _LoopbackDist(rank, world, queues, torch, gpu_lock)        # prefill uses the host-synchronised hops
            dist = _StreamLoopbackDist(rank, world, queues, torch, gpu_lock)
            eng = engines[rank]
            firsts = [D.pipeline_prefill(host, eng, rank, world, j, prompts[j], E, dev, torch.float32) for j in range(world)]
            # one throw-away row per session captures the stage graphs before the ranks run concurrently (a capture must
            # not overlap other threads' runtime calls in a shared process; separate processes do not have that problem)
            tok = torch.zeros(1, dtype=torch.int32, device=dev)
            xa, xb = (torch.zeros((1, E), dtype=torch.float32, device=dev) for _ in range(2))
            for j in range(world):
                eng.stage_step(j, tok if rank == 0 else None, None if rank == 0 else xa, prompts[0].size,
                               None if rank == world - 1 else xb, tok if rank == world - 1 else None)
            with gpu_lock:
                torch.cuda.synchronize()
            ready.wait(timeout=120)
            toks = D.pipeline_decode_streamed(dist, eng, rank, world, firsts, prompts[0].size, steps, E, dev, torch.float32)
            ready.wait(timeout=120)
            single = D.pipeline_decode_streamed(dist, eng, rank, world, firsts[:1], prompts[0].size, steps, E, dev, torch.float32, n_sessions=1)
            results[rank] = (firsts, toks, single)
        except Exception:   # noqa: BLE001
            import traceback
            errors.append((rank, traceback.format_exc()))
            ready.abort()

    # shard engines are built here, one after the other: device / context initialisation racing with other threads' allocations
    # is a property of threads-as-ranks (one HIP runtime), not of the rank-per-process launch
    engines = [LockedEngine(cfg, w, r, world, 0, n_sessions=world, max_ctx=64) for r in range(world)]
    torch.cuda.synchronize()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors[0][1]
    firsts, toks, single = results[world - 1]
    for j in range(world):
        assert firsts[j] == want[j][0]
        np.testing.assert_array_equal(toks[j], want[j][1])
    np.testing.assert_array_equal(single[0], want[0][1])


def test_stage_decode_rejects_incomplete_calls(gpu, oracle):
    """jh_stage_decode_async validates what each kind of stage needs (token word / input row / destinations)."""
    import torch
    from jlama_amd import synthetic as S
    from jlama_amd.model import HipLlamaModel
    from jlama_amd._native import JhError
    cfg = dict(S.SMALL)
    cfg["n_layers"] = 4
    w = S.make_weights(cfg, seed=2, quantize=oracle.q4_quantize)
    dev = torch.device("cuda", 0)
    E = cfg["embedding_length"]
    tok = torch.zeros(1, dtype=torch.int32, device=dev)
    x = torch.zeros((1, E), dtype=torch.float32, device=dev)
    first = HipLlamaModel(cfg, w, layer_range=(0, 2)).session(32)
    lastm = HipLlamaModel(cfg, w, layer_range=(2, 4)).session(32)
    with pytest.raises(JhError):
        first.stage_decode_async(0, 0, 0, x.data_ptr(), 0)               # first stage without a token word
    with pytest.raises(JhError):
        first.stage_decode_async(tok.data_ptr(), 0, 0, 0, 0)              # ... without a destination row
    with pytest.raises(JhError):
        lastm.stage_decode_async(0, 0, 0, 0, tok.data_ptr())              # later stage without the input row
    with pytest.raises(JhError):
        lastm.stage_decode_async(0, x.data_ptr(), 0, 0, 0)                # last stage without a token destination
    with pytest.raises(JhError):
        first.stage_decode_async(tok.data_ptr(), 0, 32, x.data_ptr(), 0)  # beyond max_ctx
    # the complete two-stage hand-off equals the un-sharded greedy step
    full = HipLlamaModel(cfg, w).session(32)
    prompt = S.prompt_tokens(cfg, n=9, seed=5)
    full.batch_forward(prompt, 0)
    f = full.sample()
    want = full.decode_n(f, prompt.size, 1)[0]
    xs = torch.zeros((prompt.size, E), dtype=torch.float32, device=dev)
    first.forward_device(prompt, 0, prompt.size, 0, xs.data_ptr())
    first.synchronize()
    lastm.forward_device(None, xs.data_ptr(), prompt.size, 0, xs.data_ptr())
    lastm.synchronize()
    tok[0] = int(f)
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    first.stage_decode_async(tok.data_ptr(), 0, prompt.size, x.data_ptr(), 0)
    first.synchronize()
    lastm.stage_decode_async(0, x.data_ptr(), prompt.size, 0, out.data_ptr())
    lastm.synchronize()
    assert int(out.item()) == int(want)


def test_rccl_world1_stream_ordered_hosts(gpu, oracle):
    """The two rank-per-GPU hosts under the REAL backend (nccl = RCCL) with a one-rank group on the test box's GPU: RCCL
    collectives issued under torch.cuda.ExternalStream(session stream) are ordered with the library's kernels.
    (a) HipTPEngine + tp_generate: a 1-shard "split" with its two all-reduces per layer equals the resident model's ids;
    (b) HipShardEngine + pipeline_decode_streamed (one stage: token word fed back on device) equals them too."""
    import socket
    import torch
    import torch.distributed as dist
    from jlama_amd import distributed as D, synthetic as S
    from jlama_amd.model import HipLlamaModel
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=dev)
    try:
        cfg = dict(S.SMALL)
        w = S.make_weights(cfg, seed=23, quantize=oracle.q4_quantize)
        prompt = S.prompt_tokens(cfg, n=10, seed=8)
        n_gen = 8
        full = HipLlamaModel(cfg, w).session(64)
        full.batch_forward(prompt, 0)
        first = full.sample()
        want = np.concatenate([[first], full.decode_n(first, prompt.size, n_gen - 1)])
        eng = D.HipTPEngine(cfg, w, 0, 1, 0, 64)
        got = D.tp_generate(dist, eng, 0, prompt, n_gen, cfg, dev, torch.float32)
        np.testing.assert_array_equal(got, want)
        E = cfg["embedding_length"]
        sh = D.HipShardEngine(cfg, w, 0, 1, 0, n_sessions=1, max_ctx=64)
        f = D.pipeline_prefill(dist, sh, 0, 1, 0, prompt, E, dev, torch.float32)
        assert f == first
        toks = D.pipeline_decode_streamed(dist, sh, 0, 1, [f], prompt.size, n_gen - 1, E, dev, torch.float32)
        np.testing.assert_array_equal(toks[0], want[1:])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("strict", [0, 1])
def test_rank_per_process_tensor_parallel_over_ipc(gpu, oracle, strict):
    """jh_tp_rank_*: one PROCESS per head-split shard (here two, both on device 0), the other rank's slot / flag / mailbox
    buffers mapped through hipIpc handles, decode = the group's token graph -- no collective on the data path.  With two shards
    the prompt's all-reduce (a + b) equals the shard-ordered sum bit for bit, so the ids must equal the one-process group's."""
    import json
    import socket
    import subprocess
    import sys
    from jlama_amd import distributed as D, synthetic as S
    from jlama_amd.model import HipLlamaModel, HipTPGroup
    n_gen = 12
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, "-m", "jlama_amd.distributed", "--tp-ipc-selftest", "--rank", str(r), "--world", "2", "--port", str(port),
                               "--n-gen", str(n_gen), "--strict", str(strict)], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=240) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    got = json.loads(outs[0][0].strip().splitlines()[-1])["ids"]
    # the same shards as a one-process group
    cfg = dict(S.SMALL)
    w = S.make_weights(cfg, seed=41)
    prompt = S.prompt_tokens(cfg, n=12, seed=7)
    models = []
    for r in range(2):
        lc, off = D.tp_shard_config(cfg, r, 2)
        models.append(HipLlamaModel(lc, D.tp_shard_weights(cfg, w, r, 2), kv_head_offset=off))
    grp = HipTPGroup(models, 96)
    for gs in grp.sessions:
        gs.set_strict(bool(strict))
    grp.forward(prompt, 0)
    first = grp.sample()
    want = [first] + list(grp.decode_n(first, prompt.size, n_gen - 1))
    grp.close()
    assert got == [int(t) for t in want]


def test_bench_tensor_parallel_leg_rank_per_process(gpu):
    """bench.py's N > 1 line under a launcher times the head-split group with ONE SHARD PER RANK (distributed.tp_rank_bench): the prompt
    in chunks through all-reduces, then the token graphs on IPC-mapped peer memory.  Here two processes on device 0 (gloo for the
    exchange): the leg must run on the graph path with no timed-out meeting, and its ids must be the one-process group's."""
    import json
    import socket
    import subprocess
    import sys
    from jlama_amd import distributed as D, synthetic as S
    from jlama_amd.model import HipLlamaModel, HipTPGroup
    n_gen = 12
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", JH_TP_SELFTEST_BENCH="1")
    procs = [subprocess.Popen([sys.executable, "-m", "jlama_amd.distributed", "--tp-ipc-selftest", "--rank", str(r), "--world", "2", "--port", str(port),
                               "--n-gen", str(n_gen), "--strict", "1"], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=240) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    leg = json.loads(outs[0][0].strip().splitlines()[-1])["leg"]
    assert leg["shards"] == 2 and leg["steps"] == n_gen - 1 and leg["single_stream_tokens_per_s"] > 0, leg
    assert leg["decode"].startswith("token graphs") and leg["ipc_error"] is None and leg["meeting_timeouts"] == 0, leg
    assert leg["prompt_rows"] == 13 and leg["prompt_rows_batched"] == 13, leg
    cfg = dict(S.SMALL)
    w = S.make_weights(cfg, seed=41)
    prompt = S.prompt_tokens(cfg, n=12, seed=7)
    models = []
    for r in range(2):
        lc, off = D.tp_shard_config(cfg, r, 2)
        models.append(HipLlamaModel(lc, D.tp_shard_weights(cfg, w, r, 2), kv_head_offset=off))
    grp = HipTPGroup(models, 96)
    for gs in grp.sessions:
        gs.set_strict(True)
    grp.forward(prompt, 0)
    first = grp.sample()
    want = [first] + list(grp.decode_n(first, prompt.size, 7))
    grp.close()
    assert leg["first_ids"] == [int(t) for t in want], (leg["first_ids"], want)


def test_one_process_bench_host_with_its_tensor_parallel_leg(gpu):
    """What a bare `python bench.py --gpus N` measures (distributed.one_process_pipeline_bench), here with two stages / two
    head-split shards on ONE device: the layer-split pipeline (single stream + N sessions in flight, all sessions agreeing)
    and the tensor-parallel group over the same devices, whose weights are generated on the first device and windowed onto
    each shard's device."""
    from jlama_amd import distributed as D
    r = D.one_process_pipeline_bench("TINY", 2, 16, 4, 8, devices=[0, 0], probe_iters=1)
    assert r["sessions"] == 2 and r["sessions_agree"] is True
    assert r["single_stream_tokens_per_s"] > 0 and r["aggregate_tokens_per_s"] > 0
    assert list(r["peer_access"]) == [None, None]                  # both hops stay on the device
    tp = r["tensor_parallel"]
    assert "error" not in tp, tp
    assert tp["shards"] == 2 and tp["steps"] == 16 and tp["single_stream_tokens_per_s"] > 0
    assert r["order"] == "order-free kernels"
    # ... and in reference order, what bench.py asks for by default (like for like with the N = 1 line's `value`)
    r2 = D.one_process_pipeline_bench("TINY", 2, 16, 4, 8, devices=[0, 0], probe_iters=1, strict=True)
    assert r2["order"].startswith("reference order") and r2["sessions_agree"] is True and "error" not in r2["tensor_parallel"], r2


@pytest.mark.parametrize("size,mode", [(2, "fast"), (4, "fast"), (2, "fast-unfused"), (2, "strict"), (4, "strict"), (2, "strict-unfused")])
def test_tensor_parallel_group_fused_reduce_loopback(gpu, oracle, monkeypatch, size, mode):
    """f2: jh_tp_group_* -- all head-split shards in one process (here on one device), the two reductions of a layer as
    one-shot slot writes + local sums in shard order, nothing synchronised on the host inside a layer.  Bit-identical to
    the same shards driven by hand with the partials summed in shard order (the path test_tensor_parallel_shards_loopback
    checks against the oracle's lock-step restatement), and greedy decode through the group equals decode by hand.
    Decode replays one graph per shard and token in which the o-proj / down GEMVs push their partial rows into every shard's
    slot themselves (EPI_TP); "-unfused" keeps the separate scatter launch (JH_TP_FUSE=0), "strict" runs the reference-order
    kernels -- every combination must give the hand loop's bits."""
    import torch
    _N.set_option("JH_TP_FUSE", "0" if mode.endswith("unfused") else "1")
    _N.set_option("JH_TP_LOUD", "1")      # a wait that times out is an error here, not a silent fall-back to the event loop
    strict = mode.startswith("strict")
    from jlama_amd import distributed as D, synthetic as S
    from jlama_amd.model import HipLlamaModel, HipTPGroup
    cfg = dict(S.SMALL)
    cfg["n_kv_heads"] = 4 if size == 4 else cfg["n_kv_heads"]      # 4 shards need >= 4 kv heads (JlamaService.java:65-68)
    w = S.make_weights(cfg, seed=41, quantize=oracle.q4_quantize)
    prompt = S.prompt_tokens(cfg, n=12, seed=7)
    E, L = cfg["embedding_length"], cfg["n_layers"]
    models, osess = [], []
    for r in range(size):
        lc, off = D.tp_shard_config(cfg, r, size)
        sw = D.tp_shard_weights(cfg, w, r, size)
        models.append(HipLlamaModel(lc, sw, kv_head_offset=off))
        osess.append(oracle.OracleModel(lc, sw, kv_head_offset=off).session())
    # (shards that meet in kernels must not share a hardware queue: the group gives same-device shards CU-masked streams)
    grp = HipTPGroup(models, 64)
    for gs in grp.sessions:
        gs.set_strict(strict)
    # by hand: partials summed in shard order on the host side of the ABI
    hand = [m.session(64) for m in models]
    for hs in hand:
        hs.set_strict(strict)
    dev = torch.device("cuda", 0)
    part = [torch.empty(E, dtype=torch.float32, device=dev) for _ in range(size)]

    def hand_row(tok, pos):
        for s in hand:
            s.tp_set_row(int(tok), pos)
        for li in range(L):
            for s, p in zip(hand, part):
                s.tp_attn(li, p.data_ptr()); s.synchronize()
            red = part[0].clone()
            for p in part[1:]:
                red = red + p
            torch.cuda.synchronize()
            for s, p in zip(hand, part):
                s.tp_ffn(li, red.data_ptr(), p.data_ptr()); s.synchronize()
            red2 = part[0].clone()
            for p in part[1:]:
                red2 = red2 + p
            torch.cuda.synchronize()
            for s in hand:
                s.tp_finish_layer(red2.data_ptr()); s.synchronize()
        return hand[0].current_row()

    def hand_rows(tokens, pos):
        """the chunk form of hand_row: [rows, E] partials, summed in shard order, once per half-layer"""
        n = len(tokens)
        parts = [torch.empty((n, E), dtype=torch.float32, device=dev) for _ in range(size)]
        for s in hand:
            s.tp_set_rows(tokens, pos)
        for li in range(L):
            for s, p in zip(hand, parts):
                s.tp_attn_rows(li, p.data_ptr()); s.synchronize()
            red = parts[0].clone()
            for p in parts[1:]:
                red = red + p
            torch.cuda.synchronize()
            for s, p in zip(hand, parts):
                s.tp_ffn_rows(li, red.data_ptr(), p.data_ptr()); s.synchronize()
            red2 = parts[0].clone()
            for p in parts[1:]:
                red2 = red2 + p
            torch.cuda.synchronize()
            for s in hand:
                s.tp_finish_layer_rows(red2.data_ptr()); s.synchronize()
        for s in hand:
            s.tp_finish_rows(); s.synchronize()
        return hand[0].current_row()

    # the prompt: one chunk of rows where the shards' shapes have the batched path (one meeting per half-layer for all 13 rows),
    # row by row otherwise -- the group and the hand loop take the same path and must agree bit for bit
    batched = all(s.tp_rows_max() >= prompt.size for s in hand)
    if batched:
        last_row = hand_rows(prompt, 0)
        if strict:                       # reference order: the chunk form IS the row form, bit for bit (KV pages included, see decode below)
            chk = [m.session(64) for m in models]
            hand, keep = chk, hand
            for hs in hand:
                hs.set_strict(True)
            by_row = [hand_row(t, i) for i, t in enumerate(prompt)][-1]
            np.testing.assert_array_equal(last_row, by_row)
            hand = keep
    else:
        last_row = [hand_row(t, i) for i, t in enumerate(prompt)][-1]
    # SMALL in halves has the batched path in both modes; in quarters its projections are too narrow for the reference-order GEMM
    assert batched == (size == 2 or not strict)
    grp.forward(prompt, 0)
    for s in grp.sessions:
        np.testing.assert_array_equal(s.current_row(), last_row)          # every shard: the same residual stream, same bits
    want_tp = oracle.forward_tp(osess, prompt, 0)
    assert _rel(last_row, want_tp[-1]) <= TRUNK_TOL
    if strict:
        np.testing.assert_array_equal(last_row, want_tp[-1])              # reference order: the lock-step oracle's bits (jo_forward_tp)
    first = grp.sample()
    assert first == hand[0].sample()
    # Shards that meet in kernels need a hardware queue each and CUs the other shards' waiting kernels cannot occupy: on ONE device
    # the group gives every shard a CU-masked stream (jh_tp_group_create), so the graph loop must work at the first attempt --
    # JH_TP_LOUD turns a timed-out meeting into an error instead of a reported fallback.
    got = grp.decode_n(first, prompt.size, 10)
    st = grp.status()
    assert st["timeouts"] == 0 and st["mode"].startswith("graph replay"), st
    tok, want_ids = first, []
    for i in range(10):
        hand_row(tok, prompt.size + i)
        tok = hand[0].sample()
        want_ids.append(tok)
    np.testing.assert_array_equal(got, np.array(want_ids, dtype=np.int32))
    grp.close()
