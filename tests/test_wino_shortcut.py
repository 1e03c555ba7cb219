"""conv_block_1 of the learned-shortcut SPADE res blocks in the Winograd domain, the 1x1 shortcut as extra K columns of the
batched GEMM at the centre-tap positions.

CPU: the algebra the fusion rests on, in fp64 numpy, with the transform matrices of the kernels (F(2x2, 3x3) with the
points {0, +-1, inf}; F(4x4, 3x3) with {0, +-3/4, +-3/2, inf}), and the launch plan with the path on and off.
GPU: with the path off (RIB_NO_WINO_SHORTCUT=1), forced on with either tile (RIB_WINO_SHORTCUT_M=2 / 4) and as the tuned
table switches it, the blocks agree with the oracle and with the committed reference fixtures to the 2e-4 of the other
fp32 fixture tests; runs are bit-identical; a sample's frame does not depend on its batch under rib_set_plan_batch."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import _native, synth

TOL = 2e-4
BLOCKS = ("down_3", "down_4", "up_4", "up_3")
MID_CFG = dict(num_filters=16, max_num_filters=64,
               mask=dict(num_filters=32, max_num_filters=64),
               embed=dict(num_filters=32, max_num_filters=64))
MODES = {"off": {"RIB_NO_WINO_SHORTCUT": "1"}, "m2": {"RIB_WINO_SHORTCUT_M": "2"}, "m4": {"RIB_WINO_SHORTCUT_M": "4"}, "table": {}}

# F(2x2, 3x3)
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
# F(4x4, 3x3), interpolation points {0, +-3/4, +-3/2, inf} (kernels.hip.h: kWino4BT / kWino4AT; rib.hip: k_wino_filters)
G4 = np.array([[64 / 81, 0, 0], [-128 / 243, -32 / 81, -8 / 27], [-128 / 243, 32 / 81, -8 / 27],
               [32 / 243, 16 / 81, 8 / 27], [32 / 243, -16 / 81, 8 / 27], [0, 0, 1]], np.float64)
BT4 = np.array([[81 / 64, 0, -45 / 16, 0, 1, 0], [0, -27 / 16, -9 / 4, 3 / 4, 1, 0], [0, 27 / 16, -9 / 4, -3 / 4, 1, 0],
                [0, -27 / 32, -9 / 16, 3 / 2, 1, 0], [0, 27 / 32, -9 / 16, -3 / 2, 1, 0], [0, 81 / 64, 0, -45 / 16, 0, 1]], np.float64)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 3 / 4, -3 / 4, 3 / 2, -3 / 2, 0], [0, 9 / 16, 9 / 16, 9 / 4, 9 / 4, 0],
                [0, 27 / 64, -27 / 64, 27 / 8, -27 / 8, 1]], np.float64)


@pytest.mark.parametrize("m,G,BT,AT,nonzero", [(2, G2, BT2, AT2, 4), (4, G4, BT4, AT4, 16)])
def test_a_1x1_convolution_is_the_centre_tap_of_a_winograd_3x3(m, G, BT, AT, nonzero):
    rng = np.random.default_rng(m)
    T = m + 2
    d = rng.standard_normal((T, T))
    # the transforms are a 3x3 convolution to begin with
    g = rng.standard_normal((3, 3))
    y = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T
    direct = np.array([[(g * d[i:i + 3, j:j + 3]).sum() for j in range(m)] for i in range(m)])
    assert np.abs(y - direct).max() < 1e-12
    # a filter that is zero outside the centre tap: the 1x1 convolution of the tile's own m x m pixels
    w = rng.standard_normal()
    gc = np.zeros((3, 3)); gc[1, 1] = w
    U = G @ gc @ G.T
    assert np.abs(U - w * np.outer(G[:, 1], G[:, 1])).max() < 1e-15
    nz = np.argwhere(U != 0)
    assert len(nz) == nonzero and {tuple(p) for p in nz} == {(r, q) for r in range(1, m + 1) for q in range(1, m + 1)}
    V = BT @ d @ BT.T
    Vs = np.zeros_like(V); Vs[1:m + 1, 1:m + 1] = V[1:m + 1, 1:m + 1]      # V is needed at those positions only
    y = AT @ (U * Vs) @ AT.T
    assert np.abs(y - w * d[1:m + 1, 1:m + 1]).max() < 1e-12
    # and those positions of V read the tile's own pixels only (no halo): rows / columns 1..m of B^T touch d[1..m]
    assert not BT[1:m + 1, [0, T - 1]].any()
    # both ride in ONE accumulation: main 3x3 + shortcut 1x1 = A^T [U.V + U_s.V_s] A
    d2 = rng.standard_normal((T, T))
    V2 = BT @ d2 @ BT.T
    y = AT @ ((G @ g @ G.T) * V + U * V2) @ AT.T
    assert np.abs(y - (direct + w * d2[1:m + 1, 1:m + 1])).max() < 1e-12


def _host_launches(lib, B, H, W, choices=()):
    spec = rib.GenSpec.from_cfg(rib.hsm_gen_config())
    c = _native.RibConfig(**{n: getattr(spec, n) for n, _ in _native.RibConfig._fields_})
    h = C.c_void_p()
    assert lib.rib_create(C.byref(c), -1, C.byref(h)) == 0
    for name, idx in choices:
        assert lib.rib_set_choice(h, B, H, W, name.encode(), idx, 1) == 0
    n = lib.rib_num_launches(h, B, H, W)
    assert n > 0, lib.rib_last_error(h)
    buf = C.create_string_buffer(600)
    out = []
    for i in range(n):
        assert lib.rib_debug_launch_info(h, B, H, W, i, buf, 600) == 0
        name, kclass, grid, tile, flops, nbytes = buf.value.decode().split("|")
        out.append((name, grid, tile, float(flops), float(nbytes)))
    fl = (C.c_double * len(_native.KC_NAMES))()
    assert lib.rib_forward_flops(h, B, H, W, fl) == 0
    lib.rib_destroy(h)
    return out, list(fl)


def _dma_variant(lib):
    g = (C.c_int * 12)()
    for i in range(lib.rib_num_variants()):
        if lib.rib_variant_info(i, g) == 0 and g[0] == 0 and (g[1], g[2], g[4]) == (2, 2, 1):      # the 64x64 k_gemm_dma tile, fp32
            return i
    raise AssertionError("no 64x64 k_gemm_dma tile")


def test_launch_plan_with_the_shortcut_in_the_winograd_domain(monkeypatch):
    lib = _native.lib()
    for k in ("RIB_NO_WINO_SHORTCUT", "RIB_WINO_SHORTCUT_M"):
        monkeypatch.delenv(k, raising=False)
    base, fl_base = _host_launches(lib, 1, 512, 448)           # a shape without tuned entries: the cost model keeps the direct launches
    names = [o[0] for o in base]
    for b in BLOCKS:
        assert b + ".conv_block_1" in names and b + ".1.spade.modulate" in names and b + ".conv_block_1.wino_in" not in names
    # a table entry for the layer's batched GEMM switches that layer, and only that layer
    v = _dma_variant(lib)
    one, fl_one = _host_launches(lib, 1, 512, 448, [("down_4.conv_block_1.wino", v)])
    n1 = [o[0] for o in one]
    assert "down_4.conv_block_1.wino" in n1 and "down_4.conv_block_1" not in n1 and "up_4.conv_block_1" in n1
    assert fl_one == fl_base
    monkeypatch.setenv("RIB_NO_WINO_SHORTCUT", "1")
    off, _ = _host_launches(lib, 1, 512, 448, [("down_4.conv_block_1.wino", v)])
    assert [o[:3] for o in off] == [o[:3] for o in base]
    monkeypatch.delenv("RIB_NO_WINO_SHORTCUT")
    for m in (2, 4):
        monkeypatch.setenv("RIB_WINO_SHORTCUT_M", str(m))
        on, fl_on = _host_launches(lib, 1, 512, 448)
        info = {o[0]: o for o in on}
        sfx = ".wino" if m == 2 else ".wino4"
        for b in BLOCKS:
            for gone in (".conv_block_1", ".conv_block_1.splitk_sum", ".1.spade.modulate"):
                assert b + gone not in info, b + gone
            for there in (".conv_block_1.wino_in", ".conv_block_1" + sfx, ".conv_block_1.wino_out"):
                assert b + there in info, b + there
            tile = info[b + ".conv_block_1" + sfx][2]
            assert ("wino4" in tile) == (m == 4) and "wino" in tile and "%d positions" % (m * m) in tile
        # the second set of a block's first SPADE is never stored: the launch is gone where conv_block_0 is a Winograd
        # convolution too, and modulates one set where it is not
        assert "down_4.0.spade.modulate" not in info and "up_4.0.spade.modulate" not in info
        base_info = {o[0]: o for o in base}
        if "down_3.0.spade.modulate" in info:
            assert info["down_3.0.spade.modulate"][4] < base_info["down_3.0.spade.modulate"][4]
        # algorithmic FLOPs per class do not move (the shortcut's stay in the convolution class)
        assert fl_on == fl_base
        for b in BLOCKS:
            assert info[b + ".conv_block_1" + sfx][3] == base_info[b + ".conv_block_1"][3]


# ---------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _generator(monkeypatch, mode, cfgname, seed):
    for k in ("RIB_NO_WINO_SHORTCUT", "RIB_WINO_SHORTCUT_M"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    cfg = rib.hsm_gen_config(**MID_CFG) if cfgname == "mid" else rib.hsm_gen_config()
    spec = rib.GenSpec.from_cfg(cfg)
    sd = synth.make_state_dict(spec, seed)
    G = rib.Generator(cfg).eval()
    G.load_state_dict(sd)
    return spec, sd, G


_oracle_cache = {}


def _oracle_taps(key, spec, sd, inputs):
    if key not in _oracle_cache:
        from oracle import generator_ref
        taps = {}
        oimg, omask = generator_ref.RefGenerator(spec, sd)(inputs[0], None, inputs[1], inputs[2], taps=taps)
        _oracle_cache.clear()
        _oracle_cache[key] = (oimg, omask, taps)
    return _oracle_cache[key]


def _check_against_oracle(G, spec, sd, key, B, H, W, inputs):
    label, fake, prev = inputs
    img0, mask0 = [t.clone() for t in G(label, None, fake, prev)]          # production plan: the lazy sources
    img1, mask1 = [t.clone() for t in G(label, None, fake, prev)]
    assert torch.equal(img0, img1) and torch.equal(mask0, mask1)            # two runs: the same bits
    G.enable_taps()
    img, mask = G(label, None, fake, prev)                                  # every intermediate stored: the plain sources
    torch.cuda.synchronize()
    taps = G.read_taps(B, H, W)
    G.enable_taps(False)
    oimg, omask, otaps = _oracle_taps(key, spec, sd, inputs)
    report = {}
    for k, v in taps.items():
        if k.split(".")[0] in BLOCKS:
            ref = otaps[k]
            report[k] = float((v - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    assert all(b in report for b in BLOCKS)
    report["img"] = float((img0.cpu() - oimg).abs().max()); report["mask"] = float((mask0.cpu() - omask).abs().max())
    report["img_taps"] = float((img.cpu() - oimg).abs().max()); report["mask_taps"] = float((mask.cpu() - omask).abs().max())
    print(key, {k: "%.2e" % v for k, v in report.items() if k in BLOCKS or not k.split(".")[0] in BLOCKS})
    bad = {k: v for k, v in report.items() if not v <= TOL}
    assert not bad, bad
    return img0, mask0


def _switched(G, B, H, W):
    names = [o["name"] for o in G.launch_info(B, H, W)]
    return [b for b in BLOCKS if b + ".conv_block_1.wino_in" in names], names


@gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_blocks_match_oracle_and_reference_taps_mid64(monkeypatch, mode, golden_dir, golden_report):
    rep = golden_report["mid_64"]
    spec, sd, G = _generator(monkeypatch, mode, "mid", rep["seed"])
    inputs = synth.make_inputs(spec, 1, 64, 64, rep["seed"])
    img, mask = _check_against_oracle(G, spec, sd, ("mid", 64), 1, 64, 64, inputs)
    g = np.load(os.path.join(golden_dir, "mid_64.npz"))
    s = rep["sub"]
    assert np.abs(img.cpu()[:, :, ::s, ::s].numpy() - g["img"]).max() <= TOL and np.abs(mask.cpu()[:, :, ::s, ::s].numpy() - g["mask"]).max() <= TOL
    # the reference's own layer outputs of these blocks
    G.enable_taps()
    G(*[inputs[0], None, inputs[1], inputs[2]])
    torch.cuda.synchronize()
    taps = G.read_taps(1, 64, 64)
    G.enable_taps(False)
    gt = np.load(os.path.join(golden_dir, "mid_64_taps.npz"))
    with open(os.path.join(golden_dir, "mid_64_tap_names.json")) as f:
        pairs = json.load(f)
    checked = 0
    for rn, on in pairs.items():
        if on.split(".")[0] in BLOCKS and on in taps:
            ref = gt[rn.replace(".", "__")]
            mine = taps[on]
            mine = (mine[:, :, ::2, ::2] if mine.shape[-1] >= 32 else mine).numpy()
            assert np.abs(mine - ref).max() <= TOL * max(1.0, np.abs(ref).max()), rn
            checked += 1
    assert checked >= 1


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["full_512", "full_b3_96x160"])
def test_blocks_match_oracle_and_reference_fixtures_full(monkeypatch, mode, name, golden_dir, golden_report):
    rep = golden_report[name]
    spec, sd, G = _generator(monkeypatch, mode, "full", rep["seed"])
    B, H, W = rep["B"], rep["H"], rep["W"]
    inputs = synth.make_inputs(spec, B, H, W, rep["seed"])
    on, names = _switched(G, B, H, W)
    if mode in ("m2", "m4"):
        assert on == list(BLOCKS)
    if mode == "off":
        assert on == []
    for b in on:      # what the switch removes
        assert b + ".1.spade.modulate" not in names and b + ".conv_block_1.splitk_sum" not in names and b + ".conv_block_1" not in names
    img, mask = _check_against_oracle(G, spec, sd, name, B, H, W, inputs)
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    s = rep["sub"]
    d_img = np.abs(img.cpu()[:, :, ::s, ::s].numpy() - g["img"]).max()
    d_mask = np.abs(mask.cpu()[:, :, ::s, ::s].numpy() - g["mask"]).max()
    print(name, mode, "switched", on, "img %.2e mask %.2e vs the reference fixture" % (d_img, d_mask))
    assert d_img <= TOL and d_mask <= TOL, (d_img, d_mask)


@gpu
@pytest.mark.parametrize("mode", ["m2", "m4", "table"])
def test_a_samples_frame_does_not_depend_on_its_batch(monkeypatch, mode):
    spec, sd, G = _generator(monkeypatch, mode, "full", 0)
    H = W = 512
    labels = torch.cat([synth.make_inputs(spec, 1, H, W, 70 + b)[0] for b in range(4)])[None].cuda()
    dains = torch.cat([synth.make_inputs(spec, 1, H, W, 70 + b)[1] for b in range(4)])[None].cuda()
    key = torch.cat([synth.make_inputs(spec, 1, H, W, 60 + b)[2] for b in range(4)]).cuda()
    try:
        G.set_plan_batch(1)
        if mode != "table":
            assert _switched(G, 4, H, W)[0] == list(BLOCKS)
        i4, m4, f4 = [t.clone() for t in G.chain(key, labels, dains)]
        i4b, m4b, f4b = G.chain(key, labels, dains)
        assert torch.equal(i4, i4b) and torch.equal(m4, m4b) and torch.equal(f4, f4b)
        for b in range(4):
            i1, m1, f1 = G.chain(key[b:b + 1], labels[:, b:b + 1], dains[:, b:b + 1])
            assert torch.equal(f1, f4[:, b:b + 1]) and torch.equal(m1, m4[:, b:b + 1]) and torch.equal(i1, i4[:, b:b + 1]), b
    finally:
        G.set_plan_batch(0)


@gpu
def test_the_table_switches_what_it_names_at_512(monkeypatch):
    """The launch list of the scored shape: every block the tuned table switched has lost its `.1.spade.modulate`, its direct
    conv_block_1 and that launch's split-K sum; a block without an entry keeps its direct launches."""
    from render_in_between_amd import tuning
    spec, sd, G = _generator(monkeypatch, "table", "full", 0)
    entry = tuning.load(dtype="f32").get("1,512,512", {})
    tabled = [b for b in BLOCKS if b + ".conv_block_1.wino" in entry or b + ".conv_block_1.wino4" in entry]
    on, names = _switched(G, 1, 512, 512)
    assert on == tabled
    for b in BLOCKS:
        if b in on:
            assert b + ".1.spade.modulate" not in names and b + ".conv_block_1.splitk_sum" not in names and b + ".conv_block_1" not in names
        else:
            assert b + ".conv_block_1" in names and b + ".1.spade.modulate" in names
