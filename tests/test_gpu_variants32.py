"""Every fp32 kernel variant against the default plan and the fp64 oracle, tap by tap (run with `-m gpu` on an MI355X).

An fp32 handle (use_tuning=False, debug taps on) renders one 2x48x80 frame, then again with ONE launch pinned to another
variant (rib_set_choice).  Everything upstream of that launch is the same code on the same bits, so the launch reads
bit-identical inputs (asserted: every earlier tap is bit-equal) and the tap that is its product differs from the default
plan's by another fp32 summation order only.  That tap is held to two references, element by element:

    |a - b|     <= 5e-5 * max(1, max|b|)          b: the default plan's tap ("same layer, another summation order":
                                                  the 5e-5 relation of tests/policy_common.py, at the tensor's scale)
    |a - ref64| <= 2e-4 * max(1, max|ref64|)      ref64: oracle.generator_ref.RefGenerator in double precision, the tap of
                                                  the same name (TOL of test_layer_taps_match_oracle_mid64)

and the frame to the same two bars (its values are tanh / sigmoid bounded: the scale is 1).  Neither bar is measured here.
Where a second launch follows the pinned choice name (FOLLOWERS of the CPU file), its product tap is held to both bars too
and the taps computed from it to the fp64 bar; every other tap ahead of the product stays bit-equal.
Every render, the default plan's included, is on a workspace filled with 0xFF: rib_forward clears nothing and tapped
buffers keep their offsets whatever variant is pinned, so an element that a forced variant fails to STORE would
otherwise read back the default plan's correct value.

The case list, and the proof that it reaches every fp32 variant and every pair the measured table pins, is
tests/test_variants32_cpu.py.  variants32_f32.json in REPORT_DIR ($RIB_REPORT_DIR, else test_reports/ under the working
directory) records per launch how many pairs ran, the largest |a - b| / bound against either reference and the share of
elements that differed at all: written, never read back."""
import ctypes as C
import json
import os

import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import _native, synth
from tests.test_variants32_cpu import (B, FMT, FOLLOWERS, GEMM_LEVELS, H, INPUT_SEED, KSPLITS, LAUNCHES, NUM_TAPS, W, WINO_GEMMS, accepted,
                                       candidates, gemm_launch, gemms, takes_choice, variants)

pytestmark = pytest.mark.gpu

TOL_AB = 5e-5                      # same layer, another summation order (policy_common.TOL_AB)
TOL_ORACLE = 2e-4                  # the HIP path against the oracle (test_gpu_parity.TOL), here against double precision
REPORT_DIR = os.environ.get("RIB_REPORT_DIR") or "test_reports"

_state = {}
_report = {}


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


def render(G, inputs):
    """One frame of SHAPE on a fresh workspace whose every byte is 0xFF (NaN in fp32); the workspace of the shape follows the
    plan (split-K slabs), so the cached one is dropped first."""
    G._ws.clear()
    G._workspace(B, H, W).fill_(0xFF)
    img, mask = G(inputs[0], None, inputs[1], inputs[2])
    return img.clone(), mask.clone()


def state():
    """The handle, the default plan's taps and frame (its first render), and the fp64 oracle's taps and frame: made once,
    never modified."""
    if not _state:
        from oracle import generator_ref
        cfg = rib.hsm_gen_config()
        spec = rib.GenSpec.from_cfg(cfg)
        sd = synth.make_state_dict(spec, 0)
        cpu_inputs = synth.make_inputs(spec, B, H, W, INPUT_SEED)
        ref = {}
        oimg, omask = generator_ref.RefGenerator(spec, sd, dtype=torch.float64)(cpu_inputs[0], None, cpu_inputs[1], cpu_inputs[2], taps=ref)
        assert oimg.dtype == torch.float64 and all(t.dtype == torch.float64 for t in ref.values())
        G = rib.Generator(cfg, use_tuning=False).eval()
        G.load_state_dict(sd)
        G.enable_taps()
        inputs = tuple(t.to(G.device) for t in cpu_inputs)
        img, mask = render(G, inputs)
        layout = tap_names(G)
        names = [n for n, _, _, _ in layout]
        _state.update(G=G, inputs=inputs, layout=layout, names=names, taps=read_taps(G, layout, len(layout)), img=img, mask=mask,
                      ref=[ref[n].to(G.device) for n in names], oimg=oimg.to(G.device), omask=omask.to(G.device))
    return _state


def ratio(a, ref, tol, scaled=True):
    """(largest |a - ref| / (tol * max(1, max|ref|)), flat index of that element); inf where a is not finite."""
    d = (a.double() - ref.double()).abs()
    r = d / (tol * (max(1.0, float(ref.abs().max())) if scaled else 1.0))
    at = int(torch.nan_to_num(r, nan=float("inf")).argmax())
    return (float(r.max()) if bool(torch.isfinite(a).all()) else float("inf")), at


def element(st, idx, got, at):
    """The worst element for a failure message: where it is and what the three sides hold there."""
    return ("flat index %d of %s: forced %.9g, default plan %.9g, fp64 %.17g"
            % (at, tuple(got.shape), float(got.flatten()[at]), float(st["taps"][idx].flatten()[at]), float(st["ref"][idx].flatten()[at])))


def write_report():
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "variants32_f32.json"), "w") as f:
        json.dump({"shape": [B, H, W], "ksplits": list(KSPLITS), "bound_default_plan": TOL_AB, "bound_fp64": TOL_ORACLE,
                   "launches": _report}, f, indent=1)


def test_default_plan_is_bit_reproducible_and_within_bounds_of_fp64():
    """The premise of the comparisons below: the plan's own choices, rendered twice on poisoned workspaces, give every tap and
    both outputs bit for bit, every element written by the run itself, every tap and the frame within 2e-4 of the fp64 oracle."""
    st = state()
    G = st["G"]
    img, mask = render(G, st["inputs"])
    taps = read_taps(G, st["layout"], len(st["layout"]))
    assert len(taps) == len(st["taps"]) == G._lib.rib_num_taps(G._h, B, H, W) == NUM_TAPS
    assert all(bool(torch.isfinite(t).all()) for t in taps) and bool(torch.isfinite(img).all()) and bool(torch.isfinite(mask).all())
    differing = [n for n, a, b in zip(st["names"], taps, st["taps"]) if not torch.equal(a, b)]
    assert not differing, differing
    assert torch.equal(img, st["img"]) and torch.equal(mask, st["mask"])
    rep = {n: ratio(a, r, TOL_ORACLE)[0] for n, a, r in zip(st["names"], taps, st["ref"])}
    rep["img"] = ratio(img, st["oimg"], TOL_ORACLE, scaled=False)[0]
    rep["mask"] = ratio(mask, st["omask"], TOL_ORACLE, scaled=False)[0]
    worst = max(rep, key=rep.get)
    print("default plan vs fp64: largest |a - ref64| / bound %.4f at %s" % (rep[worst], worst))
    _report["default plan"] = {"max_ratio_to_fp64_bound": rep[worst], "at": worst}
    write_report()
    bad = {k: v for k, v in rep.items() if not v <= 1.0}
    assert not bad, "first taps over 2e-4 * max(1, max|ref64|): %s" % list(bad.items())[:6]


def run_launch(launch, tap, every_tap=False):
    """Pins `launch` to every candidate (variant, ksplit) in turn; returns (accepted pairs, violations) and records the figures.
    every_tap: hold every tap of the run, not only `tap`, to the fp64 bound (a GEMM's slab has readers behind the first)."""
    st = state()
    G, lib = st["G"], st["G"]._lib
    idx = st["names"].index(tap)
    # a second launch that follows the pinned choice name (FOLLOWERS): its product is a product of the forced variant too,
    # and the taps computed from it are no longer upstream of anything
    _, ftap, behind = FOLLOWERS.get(launch, (None, None, ()))
    products = [idx] + ([st["names"].index(ftap)] if ftap else [])
    loose = [st["names"].index(n) for n in behind]
    igemm, tiles = variants(FMT)
    ran, faults, shares = [], [], []
    worst = {"default": 0.0, "fp64": 0.0, "frame_default": 0.0, "frame_fp64": 0.0}
    try:
        for vi, ks in candidates(launch):
            G._ws.clear()
            if not takes_choice(lib, G._h, FMT, launch, vi, ks):
                continue                                 # the plan builder refuses: does not fit this launch
            img, mask = render(G, st["inputs"])          # (an error of the run itself is not a refusal: it ends the test)
            ran.append((vi, ks))
            what = (launch, igemm.get(vi) or tiles[vi], ks)
            got = read_taps(G, st["layout"], len(st["layout"]) if every_tap else idx + 1)
            # 1. the launch read the inputs the default run's launch read
            moved = [st["names"][j] for j in range(idx) if j not in products + loose and not torch.equal(got[j], st["taps"][j])]
            if moved:
                faults.append(what + ("taps upstream of %s differ: %s" % (tap, moved[:4]),))
            # 2. its product: another summation order of the default plan's, and the fp64 oracle's value
            shares.append(float((got[idx] != st["taps"][idx]).double().mean()))
            for j in products:
                for key, ref, tol in (("default", st["taps"][j], TOL_AB), ("fp64", st["ref"][j], TOL_ORACLE)):
                    r, at = ratio(got[j], ref, tol)
                    worst[key] = max(worst[key], r)
                    if not r <= 1.0:
                        faults.append(what + ("%s: %.3f x the %g bound against %s, %s" % (st["names"][j], r, tol, key, element(st, j, got[j], at)),))
            for j in loose + list(range(idx + 1, len(got))):
                r, at = ratio(got[j], st["ref"][j], TOL_ORACLE)
                worst["fp64"] = max(worst["fp64"], r)
                if not r <= 1.0:
                    faults.append(what + ("%s: %.3f x the %g bound against fp64, %s" % (st["names"][j], r, TOL_ORACLE, element(st, j, got[j], at)),))
            # 3. the frame it leads to
            for key, a, ref, tol in (("frame_default", img, st["img"], TOL_AB), ("frame_default", mask, st["mask"], TOL_AB),
                                     ("frame_fp64", img, st["oimg"], TOL_ORACLE), ("frame_fp64", mask, st["omask"], TOL_ORACLE)):
                r, at = ratio(a, ref, tol, scaled=False)
                worst[key] = max(worst[key], r)
                if not r <= 1.0:
                    faults.append(what + ("%s of the frame: %.3f x %g (%s), flat index %d" % ("img" if a is img else "mask", r, tol, key, at),))
    finally:
        restored = lib.rib_set_choice(G._h, B, H, W, launch.encode(), -1, 1)
        G._ws.clear()
    assert restored == 0
    _report[launch] = {"tap": tap, "accepted": len(ran), "max_ratio_to_default_plan_bound": worst["default"],
                       "max_ratio_to_fp64_bound": worst["fp64"], "max_frame_ratio_to_default_plan_bound": worst["frame_default"],
                       "max_frame_ratio_to_fp64_bound": worst["frame_fp64"], "max_share_differing": max(shares) if shares else None,
                       "mean_share_differing": sum(shares) / len(shares) if shares else None}
    write_report()
    print("%s -> %s: %d pairs, ratios %s" % (launch, tap, len(ran), {k: round(v, 4) for k, v in worst.items()}))
    return ran, faults


@pytest.mark.parametrize("launch,tap", LAUNCHES)
def test_every_fp32_igemm_variant_matches_the_default_plan_and_fp64_on_its_tap(launch, tap):
    """Every fp32 k_igemm variant x split-K 1, 2, 3, 4, 8 that fits `launch`: same inputs, the product within 5e-5 of the default
    plan's and within 2e-4 of the fp64 oracle's at the tap's scale, the frame within the same two bars.  What fits is what the
    host-only plan builder accepted (tests/test_variants32_cpu.py): no pair is skipped here that was counted there."""
    ran, faults = run_launch(launch, tap)
    assert tuple(ran) == accepted(launch), (len(ran), len(accepted(launch)))
    assert ran
    assert not faults, "%d of %d runs: %s" % (len({f[:3] for f in faults}), len(ran), faults[:6])


@pytest.mark.parametrize("launch", [gemm_launch(k) for k in GEMM_LEVELS] + [name for name, _ in WINO_GEMMS])
def test_every_fp32_gemm_tile_matches_the_default_plan_and_fp64_on_its_tap(launch):
    """Each of the five fp32 k_gemm_dma tiles forced on a condition level's gamma/beta GEMM (its tap: the level's first SPADE
    output, an elementwise modulate with the slab) and on three Winograd position GEMMs of different M (their tap: the first
    one behind the output transform).  The named tap is held to both bars; it covers every row of a gamma/beta slab but only
    the columns of the first SPADE's first set, so every later tap of the run is held to the fp64 bar as well."""
    tap = dict(gemms(state()["layout"]))[launch]
    ran, faults = run_launch(launch, tap, every_tap=True)
    assert tuple(ran) == accepted(launch) and len(ran) == len(variants(FMT)[1]) == 5
    assert not faults, faults[:6]
