"""Every bf16 / half kernel variant against the default plan, tap by tap (run with `-m gpu` on an MI355X).

A 16-bit handle renders one 2x48x80 frame with debug taps on, then again with ONE launch pinned to another variant
(rib_set_choice).  Everything upstream of that launch is the same code on the same bits, so the launch reads bit-identical
inputs (asserted: every earlier tap is bit-equal), and its product - accumulated in fp32, split-K slabs and wave-group
reductions included - is rounded ONCE to the storage format.  On the tap that is that launch's product two correct
kernels therefore differ, element by element, by at most one step of the format plus fp32 summation-order noise:

    |a - b| <= u * max(|a|, |b|) + 5e-5 * max(1, max|b|)          a: forced variant, b: default plan

u = 2^-7 (bf16: 8 significand bits) or 2^-10 (half: 11): the largest spacing of neighbouring values relative to the value.
The additive term is the bound the fp32 variant tests put on "same launch, another tile geometry" (5e-5), at the tensor's
scale as test_layer_taps_match_oracle_mid64 scales it; it matters only where cancellation leaves a value much smaller
than its terms, and it covers half's subnormal floor.  Neither term is measured.

The case list, and the proof that it reaches every 16-bit variant and every pair the measured table pins, is
tests/test_variants16_cpu.py.  variants16_<fmt>.json in REPORT_DIR ($RIB_REPORT_DIR, else test_reports/ under the working
directory) records per launch how many pairs ran, the largest |a - b| / bound and the share of elements that differed
at all: recorded, never asserted on."""
import ctypes as C
import json
import os

import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import _native, synth
from tests.test_gpu_parity import BF16_MAX_IMG, BF16_MAX_MASK, F16_MAX, oracle
from tests.test_variants16_cpu import (B, GEMM_LEVELS, H, INPUT_SEED, LAUNCHES, NUM_TAPS, W, accepted, candidates, gemm_launch,
                                       gemm_tap, gemm_taps, takes_choice, variants)

pytestmark = pytest.mark.gpu

U = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10}
ADD = 5e-5
MAX_TRIPWIRE = {"bf16": (BF16_MAX_IMG, BF16_MAX_MASK), "f16": (F16_MAX, F16_MAX)}      # (img, mask): the frame tests' constants
MEAN_BAND = (0.8, 1.2)            # _assert_on_rounding_model's band on the mean error (its max band is a tail statistic: not here)
FMTS = ("bf16", "f16")
REPORT_DIR = os.environ.get("RIB_REPORT_DIR") or "test_reports"

_shared = {}
_state = {}
_report = {fmt: {} for fmt in FMTS}


def shared():
    """Checkpoint, inputs and the fp32 oracle's frame: once for both precisions."""
    if not _shared:
        cfg = rib.hsm_gen_config()
        spec = rib.GenSpec.from_cfg(cfg)
        sd = synth.make_state_dict(spec, 0)
        inputs = synth.make_inputs(spec, B, H, W, INPUT_SEED)
        label, fake, prev = inputs
        oimg, omask = oracle(spec, sd)(label, None, fake, prev)
        _shared.update(cfg=cfg, spec=spec, sd=sd, inputs=inputs, oimg=oimg.cuda(), omask=omask.cuda())
    return _shared


def tap_names(G):
    name = C.c_char_p(); ch = C.c_int(); th = C.c_int(); tw = C.c_int()
    out = []
    for i in range(G._lib.rib_num_taps(G._h, B, H, W)):
        _native.check(G._h, G._lib.rib_tap_info(G._h, B, H, W, i, C.byref(name), C.byref(ch), C.byref(th), C.byref(tw)))
        out.append((name.value.decode(), ch.value, th.value, tw.value))
    return out


def read_taps(G, layout, count):
    """The first `count` taps of the last forward, in plan order, as device tensors."""
    ws = G._workspace(B, H, W)
    out = []
    for i, (_, ch, th, tw) in enumerate(layout[:count]):
        dst = torch.empty((B, ch, th, tw), dtype=torch.float32, device=G.device)
        _native.check(G._h, G._lib.rib_read_tap(G._h, B, H, W, i, C.c_void_p(ws.data_ptr()), C.c_void_p(dst.data_ptr()), G._stream()))
        out.append(dst)
    return out


def frame_error(img, mask):
    s = shared()
    di, dm = (img - s["oimg"]).abs(), (mask - s["omask"]).abs()
    return {"max_abs_img": float(di.max()), "mean_abs_img": float(di.mean()), "max_abs_mask": float(dm.max()), "mean_abs_mask": float(dm.mean())}


def frame_faults(fmt, model, img, mask):
    """What a rendered frame breaks of: finite; the frame tests' tripwire maxima; mean error on the rounding model."""
    if not (bool(torch.isfinite(img).all()) and bool(torch.isfinite(mask).all())):
        return ["frame not finite"]
    e = frame_error(img, mask)
    bad = []
    for k, lim in zip(("max_abs_img", "max_abs_mask"), MAX_TRIPWIRE[fmt]):
        if not e[k] <= lim:
            bad.append("%s %.3e > %.3e" % (k, e[k], lim))
    for k in ("mean_abs_img", "mean_abs_mask"):
        if not MEAN_BAND[0] <= e[k] / model[k] <= MEAN_BAND[1]:
            bad.append("%s %.3e is %.3f x the model's %.3e" % (k, e[k], e[k] / model[k], model[k]))
    return bad


def state(fmt):
    """One handle per precision, taps on, with the default plan's taps and frame and the rounding model's prediction."""
    if fmt not in _state:
        from oracle import precision_model
        s = shared()
        G = rib.Generator(s["cfg"], use_tuning=False, compute_dtype=fmt).eval()
        G.load_state_dict(s["sd"])
        G.enable_taps()
        label, fake, prev = [t.to(G.device) for t in s["inputs"]]
        img, mask = G(label, None, fake, prev)
        layout = tap_names(G)
        _state[fmt] = dict(G=G, inputs=(label, fake, prev), layout=layout, names=[n for n, _, _, _ in layout],
                           taps=read_taps(G, layout, len(layout)), img=img.clone(), mask=mask.clone(),
                           model=precision_model.predict(s["spec"], s["sd"], *s["inputs"], fmt=fmt))
    return _state[fmt]


def poisoned_workspace(G):
    """The workspace the next render of SHAPE uses, every byte 0xFF: NaN in fp32, bf16 and half.  rib_forward clears nothing,
    tapped buffers keep their offsets whatever variant is pinned, and a freed workspace comes back from the allocator with
    the previous render's bytes: without this an element that a launch fails to STORE would read back the earlier,
    correct value."""
    ws = G._workspace(B, H, W)
    ws.fill_(0xFF)
    return ws


def write_report(fmt):
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "variants16_%s.json" % fmt), "w") as f:
        json.dump({"shape": [B, H, W], "u": U[fmt], "additive": ADD, "launches": _report[fmt]}, f, indent=1)


@pytest.mark.parametrize("fmt", FMTS)
def test_default_plan_is_bit_reproducible_and_on_the_rounding_model(fmt):
    """The premise of the bound: the plan's own choices, rendered twice, give every tap and both outputs bit for bit."""
    st = state(fmt)
    G = st["G"]
    G._ws.clear()
    poisoned_workspace(G)
    img, mask = G(st["inputs"][0], None, st["inputs"][1], st["inputs"][2])
    taps = read_taps(G, st["layout"], len(st["layout"]))
    assert len(taps) == len(st["taps"]) == G._lib.rib_num_taps(G._h, B, H, W) == NUM_TAPS
    assert all(bool(torch.isfinite(t).all()) for t in taps)          # every element of every tap is written by the run itself
    differing = [n for n, a, b in zip(st["names"], taps, st["taps"]) if not torch.equal(a, b)]
    assert not differing, differing
    assert torch.equal(img, st["img"]) and torch.equal(mask, st["mask"])
    assert not frame_faults(fmt, st["model"], img, mask)


def bound_ratio(fmt, a, ref):
    """(largest |a - b| / bound, share of elements that differ, flat index of the worst, how many over); inf where a is not finite."""
    a, ref = a.double(), ref.double()
    d = (a - ref).abs()
    ratio = d / (U[fmt] * torch.maximum(a.abs(), ref.abs()) + ADD * max(1.0, float(ref.abs().max())))
    r = float(ratio.max()) if bool(torch.isfinite(a).all()) else float("inf")
    return r, float((d > 0).double().mean()), int(torch.nan_to_num(ratio, nan=float("inf")).argmax()), int((~(ratio <= 1.0)).sum())


def run_launch(fmt, launch, tap, later=()):
    """Pins `launch` to every (variant, ksplit) of the precision in turn; returns (accepted pairs, violations) and records the figures.
    later: taps behind `tap` that read the launch's product too (gemm_taps); each is held to the same bound as long as every
    tap in front of it is bit-equal to the default run's, i.e. as long as it still carries ONE rounding of that product."""
    st = state(fmt)
    G, lib = st["G"], st["G"]._lib
    label, fake, prev = st["inputs"]
    idx = st["names"].index(tap)
    ref = st["taps"][idx]
    igemm, tiles = variants(fmt)
    ran, faults = [], []
    worst, shares, held = 0.0, [], []
    try:
        for vi, ks in candidates(fmt, launch):
            G._ws.clear()                                # the workspace of the shape follows the plan (split-K slabs)
            if not takes_choice(lib, G._h, fmt, launch, vi, ks):
                continue                                 # the plan builder refuses: does not fit this launch
            poisoned_workspace(G)
            img, mask = G(label, None, fake, prev)       # (an error of the run itself is not a refusal: it ends the test)
            ran.append((vi, ks))
            what = (launch, igemm.get(vi) or tiles[vi], ks)
            got = read_taps(G, st["layout"], len(st["layout"]) if later else idx + 1)
            # 1. the launch read the inputs the default run's launch read
            moved = [n for n, a, b in zip(st["names"][:idx], got, st["taps"]) if not torch.equal(a, b)]
            if moved:
                faults.append(what + ("taps upstream of %s differ: %s" % (tap, moved[:4]),))
            # 2. its product: one rounding of the same fp32 sum
            r, share, at, over = bound_ratio(fmt, got[idx], ref)
            worst = max(worst, r)
            shares.append(share)
            if not r <= 1.0:
                faults.append(what + ("%s: |a - b| is %.3f x the bound (a %.6g, b %.6g at flat index %d; %d elements over)"
                                      % (tap, r, float(got[idx].flatten()[at]), float(ref.flatten()[at]), at, over),))
            # 2b. the later readers of the product, while nothing in front of them has moved
            n_held = 1
            for j in range(idx + 1, len(got) if later else idx + 1):
                if not torch.equal(got[j - 1], st["taps"][j - 1]):
                    break                                # from here on a tap may carry a second rounding
                if st["names"][j] in later:
                    r, _, at, over = bound_ratio(fmt, got[j], st["taps"][j])
                    worst = max(worst, r)
                    n_held += 1
                    if not r <= 1.0:
                        faults.append(what + ("%s: |a - b| is %.3f x the bound (flat index %d; %d elements over)" % (st["names"][j], r, at, over),))
            held.append(n_held)
            # 3. the frame it leads to
            bad = frame_faults(fmt, st["model"], img, mask)
            if bad:
                faults.append(what + tuple(bad))
    finally:
        restored = lib.rib_set_choice(G._h, B, H, W, launch.encode(), -1, 1)
        G._ws.clear()
    assert restored == 0
    _report[fmt][launch] = {"tap": tap, "accepted": len(ran), "taps_held_per_run": min(held) if held else 0, "max_ratio_to_bound": worst,
                            "max_share_differing": max(shares) if shares else None,
                            "mean_share_differing": sum(shares) / len(shares) if shares else None}
    write_report(fmt)
    return ran, faults


@pytest.mark.parametrize("fmt,launch,tap", [(f, l, t) for f in FMTS for l, t in LAUNCHES])
def test_every_16_bit_igemm_variant_matches_the_default_plan_on_its_tap(fmt, launch, tap):
    """Every k_igemm variant of the precision x split-K 1..4 that fits `launch`: same inputs, the product within one step of
    the format of the default plan's, the frame still on the rounding model.  What fits is what the host-only plan builder
    accepted (tests/test_variants16_cpu.py): no pair is skipped here that was counted there."""
    ran, faults = run_launch(fmt, launch, tap)
    assert tuple(ran) == accepted(fmt, launch), (len(ran), len(accepted(fmt, launch)))
    assert ran
    assert not faults, "%d of %d runs: %s" % (len({f[:3] for f in faults}), len(ran), faults[:6])


@pytest.mark.parametrize("fmt,level", [(f, k) for f in FMTS for k in GEMM_LEVELS])
def test_every_16_bit_gemm_tile_matches_the_default_plan_on_its_tap(fmt, level):
    """Each k_gemm_dma tile forced on a condition level's gamma/beta GEMM.  Its slab is fp32; the first SPADE of the level
    modulates with it elementwise and stores the tap.  That tap covers every row of the slab (M: the pixels) but only the
    columns of N that are this SPADE's first set; the other columns belong to its second set and to the later SPADEs of the
    level.  Those SPADEs' taps are held to the same bound for as long as every tap in front of them is bit-equal (then their
    other operand is the default run's, and they too carry one rounding); the columns of a second set, which no tap stores,
    show in the block's output tap only, which must be bit-equal for the walk to go on, and in the frame checks."""
    layout = state(fmt)["layout"]
    ran, faults = run_launch(fmt, gemm_launch(level), gemm_tap(layout, level), later=gemm_taps(layout, level)[1:])
    assert tuple(ran) == accepted(fmt, gemm_launch(level)) and len(ran) == len(variants(fmt)[1]) == 4
    assert not faults, faults[:6]
