"""W13 on the device (csrc/w13.hip, csrc/vv_w13.h, the W13 forms of csrc/gemv.hip) against the definition (vibevoice_amd/w13.py) and
against the bf16 route it must reproduce bit for bit.  Equality is the whole oracle: the bf16 route is held to fp64 by
test_gpu_gemv_forms.py and the sampler tests; test_w13_cpu.py asserts that none of the normal tensors used here falls back.

  pack kernel      planes, scale words, ok words and the folded word equal w13.twin() byte for byte; the unpack kernel returns the
                   source fragments; N = 32, K = 128, 256, 384 (one group; fewer groups than waves); planted elements: the ok words of
                   the device round trip equal the rule's
  GEMV forms       each W13 form over the twins against the SAME form over the bf16 fragments, torch.equal, 2 rows: gate/up in the
                   2-row 4-wave form (H = 256: 2 groups over 4 waves) and in the default form, down in the default form (I = 1152: 9
                   groups over 8 waves of 5, 5, ..., 1 k-tiles: ranges that start and end inside a group); with and without a shift
                   operand; K = 128: waves without K.  Where the plan's own bf16 launch has the same form, it gives the same bits too
  sampler          diffusion_sample, N = 3, at both widths: latents equal between VVHIP_W13 on and off, eager and graphed;
                   vv_stat(9) = 12 when on; after re-uploading one down matrix; with one planted denormal (vv_stat(9) = 11)"""
import os

import numpy as np
import pytest
import torch

import synth
import w13_cases as WC
from gpu_util import build_small
from vibevoice_amd import w13

pytestmark = pytest.mark.gpu

NONE, RMS_MOD = 0, 2
SWIGLU, GATED = 3, 5
EPS = 1e-5


@pytest.fixture(scope="module")
def eng():
    s = build_small(synth.LMCfg(), xsplit=1)
    yield s.eng
    s.eng.close()


def _pack(eng, w):
    """bf16 [N][K] -> (packed fragments, twin), both uint8 on the device"""
    packed = eng.pack_matrix(w.float())
    twin = eng.w13_pack(packed, *w.shape)
    eng.sync()
    return packed, twin


@pytest.mark.parametrize("N,K", WC.PACK_SHAPES)
def test_pack_kernel_matches_the_definition(eng, N, K):
    w = WC.weights(N, K, 40 + K)
    b = WC.bits(w)
    packed, twin = _pack(eng, w)
    assert np.array_equal(packed.cpu().numpy().view(np.uint16).reshape(N // 16, K // 32, 64, 8), w13.fragments(b))
    assert np.array_equal(twin.cpu().numpy(), w13.twin(b))
    back = eng.w13_unpack(twin, N, K)
    eng.sync()
    assert torch.equal(back, packed)


@pytest.mark.parametrize("value,rep", [(0x0000, True), (0x8000, True), (WC.DENORMAL, False), (WC.INF, False), (WC.NAN, False), ("under31", False),
                                       ("under29", True)])
def test_the_device_round_trip_agrees_with_the_rule(eng, value, rep):
    N, K = 32, 256
    b = WC.bits(WC.weights(N, K, 5))
    if isinstance(value, str):
        row = b[16:32].reshape(-1)
        value = WC.under(row[np.argmax((row >> 7) & 0xFF)], int(value[5:]))
    b[20, 70] = value
    packed = eng.pack_matrix(WC.from_bits(b).float())
    assert np.array_equal(packed.cpu().numpy().view(np.uint16).reshape(N // 16, K // 32, 64, 8), w13.fragments(b)), "the planted bits did not survive the upload"
    twin = eng.w13_pack(packed, N, K)
    eng.sync()
    got = twin.cpu().numpy()
    assert np.array_equal(got, w13.twin(b))
    tail = got[w13.plane_bytes(N, K):].view(np.uint32)
    assert tail[2:5].tolist() == [1, int(rep), int(rep)]
    if rep:
        assert torch.equal(eng.w13_unpack(twin, N, K), packed)


_mats = {}


def _gemv_mats(eng, H, I):
    if (H, I) not in _mats:
        _mats[H, I] = {k: _pack(eng, v) for k, v in WC.gemv_weights(H, I).items()}
    return _mats[H, I]


def _rows(eng, seed, T, width, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, width, generator=g) * scale).to(eng.device)


def _gate_up(eng, H, I, form, shift, twins, mats=None, natural=False):
    m = mats or _gemv_mats(eng, H, I)
    x, sc = _rows(eng, 1, 2, H), _rows(eng, 2, 2, H, 0.3)
    sh = _rows(eng, 3, 2, H, 0.5) if shift else torch.zeros(2, H, device=eng.device)
    nw = _rows(eng, 4, 1, H).reshape(-1) * 0.1 + 1.0
    y = torch.full((2, I), 7.0, device=eng.device)
    kw = dict(pro=RMS_MOD, epi=SWIGLU, w2p=m["up"][0], nw=nw, eps=EPS, mod_scale=sc, mod_shift=sh, ld_mod=H, xsplit=1)
    if not natural:
        kw.update(w13_form=form, twin=m["gate"][1] if twins else None, twin2=m["up"][1] if twins else None)
    got = eng.gemv_case(m["gate"][0], x, y, 2, I, H, **kw)
    eng.sync()
    return got, y


def _down(eng, H, I, form, twins, mats=None, natural=False):
    m = mats or _gemv_mats(eng, H, I)
    x, gate = _rows(eng, 5, 2, I), _rows(eng, 6, 2, H, 0.5)
    y = _rows(eng, 7, 2, H).clone()
    kw = dict(pro=NONE, epi=GATED, gate=gate, ld_gate=H, xsplit=1)
    if not natural:
        kw.update(w13_form=form, twin=m["down"][1] if twins else None)
    got = eng.gemv_case(m["down"][0], x, y, 2, H, I, **kw)
    eng.sync()
    return got, y


@pytest.mark.parametrize("H,I", WC.WIDTHS)
@pytest.mark.parametrize("form", [(2, 4), (4, 8)])
@pytest.mark.parametrize("shift", [True, False])
def test_gate_up_form_gives_the_bits_of_bf16(eng, H, I, form, shift):
    f0, y0 = _gate_up(eng, H, I, form, shift, twins=False)
    f1, y1 = _gate_up(eng, H, I, form, shift, twins=True)
    assert f0 == f1 == (1, *form, 0, 0)
    assert bool(torch.isfinite(y0).all()) and float(y0.abs().max()) > 0 and not bool((y0 == 7.0).any())
    assert torch.equal(y0, y1)
    fn, yn = _gate_up(eng, H, I, None, shift, twins=False, natural=True)      # the launch the plan gives these widths
    if fn == f0:
        assert torch.equal(yn, y1)
    else:
        assert form == (2, 4) and fn == (1, 4, 8, 0, 0)


@pytest.mark.parametrize("H,I", WC.WIDTHS)
def test_down_form_gives_the_bits_of_bf16(eng, H, I):
    f0, y0 = _down(eng, H, I, (4, 8), twins=False)
    f1, y1 = _down(eng, H, I, (4, 8), twins=True)
    fn, yn = _down(eng, H, I, None, twins=False, natural=True)
    assert f0 == f1 == fn == (1, 4, 8, 0, 0)
    assert bool(torch.isfinite(y0).all()) and not torch.equal(y0, _rows(eng, 7, 2, H))
    assert torch.equal(y0, y1) and torch.equal(yn, y1)


def test_one_group_leaves_waves_without_k(eng):
    """K = 128: four k-tiles, so half of the default form's waves have no K; down with K = 128 likewise"""
    H, I = 128, 384
    mats = {k: _pack(eng, v) for k, v in {"gate": WC.weights(I, H, 11), "up": WC.weights(I, H, 12), "down": WC.weights(I, H, 13)}.items()}
    for form in ((2, 4), (4, 8)):
        _, y0 = _gate_up(eng, H, I, form, True, twins=False, mats=mats)
        _, y1 = _gate_up(eng, H, I, form, True, twins=True, mats=mats)
        assert torch.equal(y0, y1) and float(y0.abs().max()) > 0
    # down: N = I = 384 outputs over K = H = 128
    x, gate, y = _rows(eng, 5, 2, H), _rows(eng, 6, 2, I, 0.5), _rows(eng, 7, 2, I)
    outs = []
    for tw in (None, mats["down"][1]):
        yy = y.clone()
        assert eng.gemv_case(mats["down"][0], x, yy, 2, I, H, pro=NONE, epi=GATED, gate=gate, ld_gate=I, xsplit=1, w13_form=(4, 8), twin=tw) == (1, 4, 8, 0, 0)
        eng.sync()
        outs.append(yy)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], y)


def test_refusals(eng):
    """a shape without whole groups has no twin; a pair without a W13 form is refused, nothing launched"""
    assert int(eng.lib.vv_w13_twin_bytes(32, 96)) == 0 and int(eng.lib.vv_w13_twin_bytes(24, 128)) == 0
    with pytest.raises(ValueError):
        eng.w13_pack(torch.zeros(4096, dtype=torch.uint8, device=eng.device), 32, 96)
    m = _gemv_mats(eng, 256, 768)
    x, y = _rows(eng, 5, 2, 768), torch.full((2, 256), 7.0, device=eng.device)
    assert eng.gemv_case(m["down"][0], x, y, 2, 256, 768, pro=NONE, epi=0, xsplit=1, w13_form=(4, 8), twin=m["down"][1]) is None
    assert eng.gemv_case(m["down"][0], x, y, 2, 256, 768, pro=NONE, epi=GATED, gate=y.clone(), ld_gate=256, xsplit=1, w13_form=(4, 16), twin=m["down"][1]) is None
    eng.sync()
    assert bool((y == 7.0).all())


def _arm(on, H, graph):
    old = os.environ.get("VVHIP_W13")
    os.environ["VVHIP_W13"] = "1" if on else "0"
    try:
        cfg = synth.LMCfg(hidden=H, heads=2, kv_heads=1, inter=256, head_dim_override=128)
        return build_small(cfg, xsplit=1, use_graph=graph, n_slots=1, max_ctx=512, head_layers=WC.HEAD_LAYERS)
    finally:
        if old is None:
            os.environ.pop("VVHIP_W13", None)
        else:
            os.environ["VVHIP_W13"] = old


def _sample(s, H, calls):
    eng = s.eng
    eng.set_num_steps(3)
    cond, noise = _rows(eng, 21, 2, H), _rows(eng, 22, 1, 64)
    outs = []
    for _ in range(calls):          # graphed: first sight eager, then the capture, then a replay
        out = torch.zeros(1, 64, device=eng.device)
        if calls > 1:
            out = s.out_buf = getattr(s, "out_buf", out)      # one key: the same buffers every call
            out.zero_()
        eng.diffusion_sample(1, cond, noise, 1.3, out)
        eng.sync()
        outs.append(out.clone())
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    return outs[0]


@pytest.mark.parametrize("H,I", WC.WIDTHS)
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_sampler_arms_agree(H, I, graph):
    on, off = _arm(True, H, graph), _arm(False, H, graph)
    try:
        calls = 3 if graph else 1
        assert on.eng.stat(9) == 12 and off.eng.stat(9) == 0
        a, b = _sample(on, H, calls), _sample(off, H, calls)
        assert torch.equal(a, b)
        # one down matrix uploaded again with new values: its twin follows
        new = WC.reupload_down(H, I)
        for s in (on, off):
            s.eng.upload("head.layers.2.ffn.down_proj.weight", new)
        assert on.eng.stat(9) == 12
        a2, b2 = _sample(on, H, calls), _sample(off, H, calls)
        assert torch.equal(a2, b2) and not torch.equal(a2, a)
        # one denormal: that matrix keeps its bf16 launch, the others their twins
        bad = WC.bits(new)
        bad[5, 77] = WC.DENORMAL
        for s in (on, off):
            s.eng.upload("head.layers.2.ffn.down_proj.weight", WC.from_bits(bad))
        assert on.eng.stat(9) == 11 and off.eng.stat(9) == 0
        a3, b3 = _sample(on, H, calls), _sample(off, H, calls)
        assert torch.equal(a3, b3)
        if graph:
            assert on.eng.stat(5) == 0 and on.eng.stat(4) == 0
    finally:
        on.eng.close()
        off.eng.close()
