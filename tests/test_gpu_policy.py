"""Both sides of every launch-plan policy switch, held to the same frame (run with `-m gpu` on an MI355X).

The rows are policy_common.CASES (this file adds none); tests/test_policy_cpu.py proves that each changes the launch plan.
Every render here runs on a workspace filled with 0xFF, so an element that a launch reads before any launch stored it is
NaN, not the previous render's correct value.

  B1  the default fp32 plan, taps off and on: finite, and bit-equal to a render on a zero-filled workspace
  B2  taps on against taps off: bit-equal frames (the lazy SPADE sources against the stored ones, in the production plan)
  B3  rows whose two sides perform the same arithmetic: torch.equal on both outputs and on every tap
  B4  rows that change a summation order or a kernel family: frames within 5e-5 of the default plan's and both within 2e-4
      of the oracle; taps ahead of the row's first_tap bit-equal, first_tap within 5e-5 * max(1, max|ref|), later taps
      within 2e-4 * max(1, max|ref|)

policy_ab.json in REPORT_DIR ($RIB_REPORT_DIR, else test_reports/) records per row the launches changed, the first
differing tap, the largest frame difference and the largest tap difference relative to its bar: recorded, not asserted."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import policy_common as pc

pytestmark = pytest.mark.gpu

REPORT_DIR = os.environ.get("RIB_REPORT_DIR") or "test_reports"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 180

_default = {}
_report = {}


def default_renders(monkeypatch):
    """{(shape, taps): (render on a zero-filled workspace, render on a 0xFF-filled one)} of the default plan, made once by one
    handle while no switch is set."""
    if not _default:
        G = pc.handle(monkeypatch, {})
        for shape in pc.SHAPES + (pc.XCD_SHAPE,):
            for taps in ((False,) if shape == pc.XCD_SHAPE else (False, True)):
                _default[(shape, taps)] = (pc.render(G, shape, taps, pc.ZERO), pc.render(G, shape, taps, pc.POISON))
    return _default


def record(case_id, **figures):
    _report.setdefault(case_id, {}).update(figures)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "policy_ab.json"), "w") as f:
        json.dump({"bars": {"a_b": pc.TOL_AB, "oracle": pc.TOL_ORACLE}, "cases": _report}, f, indent=1)


def finite(*tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors)


def frame_diff(a, b):
    return max(float((a.img - b.img).abs().max()), float((a.mask - b.mask).abs().max()))


def oracle_error(shape, r):
    s = pc.shared(shape)
    return max(float((r.img - s["oimg"]).abs().max()), float((r.mask - s["omask"]).abs().max()))


def changed(base, other):
    come, gone, retiled = pc.diff(base.launches, other.launches)
    return {"come": len(come), "gone": len(gone), "retiled": len(retiled), "first": (come + gone + retiled)[:3]}


def assert_bit_equal(a, b, what):
    """Both outputs, and every tap by name, of two renders."""
    ok = finite(a.img, a.mask, b.img, b.mask)
    assert ok, what
    assert sorted(a.names) == sorted(b.names)
    mine = dict(zip(a.names, a.taps))
    differing = [n for n, t in zip(b.names, b.taps) if not torch.equal(mine[n], t)]      # in b's plan order: the first is the first
    assert not differing, (what, "first differing taps", differing[:6])
    same = torch.equal(a.img, b.img) and torch.equal(a.mask, b.mask)
    assert same, (what, "largest frame difference", frame_diff(a, b))


# ---- B1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [False, True], ids=["taps_off", "taps_on"])
@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_default_plan_reads_nothing_it_did_not_write(monkeypatch, shape, taps):
    zero, poisoned = default_renders(monkeypatch)[(shape, taps)]
    assert finite(poisoned.img, poisoned.mask)
    assert finite(*poisoned.taps) and len(poisoned.taps) == (68 if taps else 0)
    assert_bit_equal(poisoned, zero, "0xFF-filled against zero-filled workspace")
    assert oracle_error(shape, poisoned) <= pc.TOL_ORACLE


# ---- B2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_taps_on_renders_the_production_plans_frame(monkeypatch, shape):
    """With taps on every SPADE output is stored by k_spade_modulate and lives to the end of the forward; the production plan
    computes four of them inside Winograd input transforms and reuses every address."""
    d = default_renders(monkeypatch)
    off, on = d[(shape, False)][1], d[(shape, True)][1]
    come, _, _ = pc.diff(off.launches, on.launches)
    assert len(come) == 4, come
    assert torch.equal(off.img, on.img) and torch.equal(off.mask, on.mask), frame_diff(off, on)
    record("taps_on-%dx%dx%d" % shape, relation="bit", launches=changed(off, on), max_frame_diff=frame_diff(off, on))


# ---- B3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in pc.cases("bit") if not c.change.get("xcd")], ids=lambda c: c.id)
def test_switches_that_keep_the_arithmetic_keep_every_bit(monkeypatch, case):
    d = default_renders(monkeypatch)
    G = pc.handle(monkeypatch, case.env)
    for taps in (False, True):
        base = d[(case.shape, taps)][1]
        r = pc.render(G, case.shape, taps)
        what = changed(base, r)
        if not case.change.get("same"):
            assert what["come"] + what["gone"] > 0, (case.id, taps)
        record(case.id, relation="bit", **{"launches_taps_%s" % ("on" if taps else "off"): what, "max_frame_diff_taps_%s" % ("on" if taps else "off"): frame_diff(r, base)})
        first = next((n for n, t in zip(base.names, base.taps) if not torch.equal(dict(zip(r.names, r.taps))[n], t)), None)
        record(case.id, first_differing_tap=first)
        assert_bit_equal(r, base, (case.id, "taps on" if taps else "taps off"))


def test_workspace_reuse_keeps_every_bit_of_a_chain(monkeypatch):
    """One segment of three frames at batch 1: the chain's workspace, the unpaired twin of the frame plan and the labels-only
    plan, each with every buffer at its own address against the lifetime-based placement."""
    shape = pc.SHAPES[0]
    base = [t.clone() for t in pc.render_chain(pc.handle(monkeypatch, {}), shape)]
    assert finite(*base)
    zero = pc.render_chain(pc.handle(monkeypatch, {}), shape, fill=pc.ZERO)
    assert all(torch.equal(a, b) for a, b in zip(base, zero))
    got = pc.render_chain(pc.handle(monkeypatch, {"RIB_NO_WS_REUSE": "1"}), shape)
    assert finite(*got)
    diffs = [float((a - b).abs().max()) for a, b in zip(got, base)]
    record("ws_reuse-chain-T%d-%dx%dx%d" % ((pc.CHAIN_T,) + shape), relation="bit", max_frame_diff=max(diffs))
    assert all(torch.equal(a, b) for a, b in zip(got, base)), diffs


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name,shape", [("ws_reuse", pc.SHAPES[1]), ("pair", pc.SHAPES[0])])
def test_addresses_and_pairing_keep_every_bit_in_the_16_bit_modes(monkeypatch, name, shape, fmt):
    case = next(c for c in pc.CASES if c.id == "%s-%dx%dx%d" % ((name,) + shape))
    G = pc.handle(monkeypatch, {}, fmt)
    base = {taps: pc.render(G, shape, taps) for taps in (False, True)}
    G = pc.handle(monkeypatch, case.env, fmt)
    for taps in (False, True):
        r = pc.render(G, shape, taps)
        if not case.change.get("same"):
            assert changed(base[taps], r)["gone"] > 0
        record("%s-%s" % (case.id, fmt), relation="bit", **{"max_frame_diff_taps_%s" % ("on" if taps else "off"): frame_diff(r, base[taps])})
        assert_bit_equal(r, base[taps], (case.id, fmt, taps))


@pytest.mark.parametrize("case", [c for c in pc.cases("bit") if c.change.get("xcd")], ids=lambda c: c.id)
def test_the_tile_order_keeps_every_bit(monkeypatch, tmp_path, case):
    """RIB_NO_XCD is read once per process: the switched side renders in a fresh child process, started once."""
    base = default_renders(monkeypatch)[(case.shape, False)][1]
    assert len(pc.reordered_by_xcd(base.launches)) >= 8
    env = {k: v for k, v in os.environ.items() if k not in pc.POLICY_VARS}
    env.update(case.env)
    done = subprocess.run([sys.executable, "-m", "tests.policy_common", str(tmp_path)], cwd=ROOT, env=env, timeout=CHILD_TIMEOUT_S,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")[-2000:]
    got = torch.load(os.path.join(str(tmp_path), "xcd_off.pt"))
    img, mask = got["img"].cuda(), got["mask"].cuda()
    assert finite(img, mask)
    diff = max(float((img - base.img).abs().max()), float((mask - base.mask).abs().max()))
    record(case.id, relation="bit", reordered_launches=len(pc.reordered_by_xcd(base.launches)), max_frame_diff=diff)
    assert torch.equal(img, base.img) and torch.equal(mask, base.mask), diff


# ---- B4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.cases("5e-5"), ids=lambda c: c.id)
def test_switches_that_change_a_summation_stay_within_the_suites_bars(monkeypatch, case):
    d = default_renders(monkeypatch)
    G = pc.handle(monkeypatch, case.env)
    # taps off: the frames
    base, r = d[(case.shape, False)][1], pc.render(G, case.shape, False)
    what = changed(base, r)
    assert what["come"] + what["gone"] + what["retiled"] > 0
    fd = frame_diff(r, base) if finite(r.img, r.mask) else float("inf")
    eo = (oracle_error(case.shape, base), oracle_error(case.shape, r))
    record(case.id, relation="5e-5", launches=what, max_frame_diff=fd, oracle_error_default=eo[0], oracle_error_switched=eo[1])
    # taps on: the walk
    tbase, tr = d[(case.shape, True)][1], pc.render(G, case.shape, True)
    assert tr.names == tbase.names and case.first_tap in tr.names
    at = tr.names.index(case.first_tap)
    faults, worst, first = [], 0.0, None
    for i, (n, a, b) in enumerate(zip(tr.names, tr.taps, tbase.taps)):
        if torch.equal(a, b):
            continue
        first = first or n
        if i < at:
            faults.append((n, "differs ahead of %s" % case.first_tap))
            continue
        bar = (pc.TOL_AB if i == at else pc.TOL_ORACLE) * max(1.0, float(b.abs().max()))
        ratio = float((a - b).abs().max()) / bar if finite(a) else float("inf")
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            faults.append((n, "%.3f x its bar %.3e" % (ratio, bar)))
    tfd = frame_diff(tr, tbase) if finite(tr.img, tr.mask) else float("inf")
    record(case.id, first_differing_tap=first, max_tap_ratio_to_bar=worst, max_frame_diff_taps_on=tfd)
    assert fd <= pc.TOL_AB, (case.id, fd)
    assert eo[0] <= pc.TOL_ORACLE and eo[1] <= pc.TOL_ORACLE, eo
    assert not faults, faults[:6]
    assert tfd <= pc.TOL_AB, (case.id, tfd)
