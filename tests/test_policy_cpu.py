"""The launch-plan side of the policy-switch A/B (tests/test_gpu_policy.py): on host-only handles, every row of
policy_common.CASES changes the launch list in the way it names, so that no GPU comparison is between two identical plans,
and the tap at which a row lets a difference begin is the first one a differing launch can reach.  CPU only."""
import os
import re

import pytest

from tests import policy_common as pc

# switches of the plan that have an A/B test elsewhere (tests/test_gpu_parity.py, tests/test_wino_shortcut.py), and the one
# whose variants are forced tile by tile there (RIB_NO_DMA)
HELD_ELSEWHERE = {"RIB_NO_WINO", "RIB_WINO_M", "RIB_NO_LOWC", "RIB_LOWC_TW", "RIB_NO_HEADCONV", "RIB_NO_SMALLCONV", "RIB_NO_LABEL_BATCH",
                  "RIB_NO_SPADE16", "RIB_NO_WINO_SHORTCUT", "RIB_WINO_SHORTCUT_M", "RIB_NO_DMA"}
WINO_SUFFIXES = (".wino_in", ".wino", ".wino4", ".wino_out")


def both(monkeypatch, case, taps=False):
    return pc.host_plan(monkeypatch, case.base, case.shape, taps), pc.host_plan(monkeypatch, case.env, case.shape, taps)


def matches(names, patterns, what, may=()):
    assert names, what
    stray = [n for n in names if not any(p in n for p in tuple(patterns) + tuple(may))]
    assert not stray, (what, stray)
    for p in patterns:
        assert any(p in n for n in names), (what, p)


def check_counts(names, ch, key):
    if "n_" + key in ch:
        assert len(names) == ch["n_" + key], (key, len(names), names)
    assert ch.get("min_" + key, 0) <= len(names) <= ch.get("max_" + key, 10 ** 6), (key, len(names))


def check_change(case, base, other):
    ch = case.change
    come, gone, retiled = pc.diff(base.launches, other.launches)
    if ch.get("same"):
        assert other.launches == base.launches
        assert (other.ws_bytes > base.ws_bytes) if ch.get("ws_larger") else (other.ws_bytes == base.ws_bytes)
        return
    assert other.launches != base.launches
    for key, names in (("come", come), ("gone", gone)):
        if key in ch:
            matches(names, ch[key], (case.id, key), ch.get(key + "_may", ()))
            check_counts(names, ch, key)
        else:
            assert not names, (case.id, key, names)
    if "retile_gone_bases" in ch:      # the launch a gone one belonged to stays, with another kernel choice
        bases = {n.rsplit(".", 1)[0] for n in gone if n.endswith(ch["gone"][-1])}
        assert bases and bases <= set(retiled), (case.id, sorted(bases - set(retiled)))
        tiles = {n: t for n, _, t in other.launches}
        assert all(ch["retile_gone_bases"] in tiles[n] for n in bases)
    else:
        assert len(retiled) == ch.get("retile", 0), (case.id, retiled)


@pytest.mark.parametrize("case", [c for c in pc.CASES if not (c.change.get("xcd") or c.change.get("wino_threshold"))], ids=lambda c: c.id)
def test_the_switch_changes_the_plan_as_its_row_says(monkeypatch, case):
    base, other = both(monkeypatch, case)
    check_change(case, base, other)
    tb, to = both(monkeypatch, case, taps=True)
    if case.relation == "plan":
        return
    # the taps the GPU test compares exist on both sides (the unpaired encoders list theirs in another order)
    assert sorted(tb.taps) == sorted(to.taps) and len(tb.taps) == 68
    if case.relation == "5e-5":
        assert [t[0] for t in tb.taps] == [t[0] for t in to.taps]
        assert pc.first_tap(tb.launches, to.launches, case.ignore) == case.first_tap
        assert case.first_tap in [t[0] for t in tb.taps]
        check_change(case._replace(change={k: v for k, v in case.change.items() if not k.startswith(("n_", "min_", "max_"))}), tb, to)
    else:
        assert tb.launches != to.launches or to.ws_bytes > tb.ws_bytes      # with taps on the two sides still differ
        assert case.first_tap is None


def test_lazy_sources_with_and_without_taps(monkeypatch):
    """What taps-on against taps-off compares (B2 of the GPU file): with taps on every SPADE source is stored, the mask
    network's joins stay lazy (their consumer's transform stores them); RIB_NO_LAZY with taps on stores those too."""
    for shape in pc.SHAPES:
        off, on = pc.host_plan(monkeypatch, {}, shape), pc.host_plan(monkeypatch, {}, shape, taps=True)
        come, gone, _ = pc.diff(off.launches, on.launches)
        assert len(come) == 4 and all(n.endswith(".spade.modulate") for n in come) and not gone
        no_lazy = pc.host_plan(monkeypatch, {"RIB_NO_LAZY": "1"}, shape, taps=True)
        come, gone, _ = pc.diff(on.launches, no_lazy.launches)
        assert len(come) == 3 and all(n.endswith(".join") for n in come) and not gone


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.change.get("wino_threshold")], ids=lambda c: c.id)
def test_the_winograd_threshold_is_inclusive(monkeypatch, case):
    base = pc.host_plan(monkeypatch, {}, case.shape)
    dims = {n: h * w for n, _, h, w in pc.host_plan(monkeypatch, {}, case.shape, taps=True).taps}
    wino = {n: dims[pc.tap_of_launch(n)] for n, _, _ in base.launches if n.endswith(WINO_SUFFIXES)}
    assert len(wino) == 45
    largest = max(wino.values())
    assert pc.host_plan(monkeypatch, {"RIB_WINO_MAX_PX": str(largest)}, case.shape).launches == base.launches
    below = pc.host_plan(monkeypatch, {"RIB_WINO_MAX_PX": str(largest - 1)}, case.shape)
    come, gone, _ = pc.diff(base.launches, below.launches)
    assert {n for n in gone if n.endswith(WINO_SUFFIXES)} == {n for n, px in wino.items() if px == largest}
    assert 0 < len([n for n in gone if n.endswith(".wino_in")]) < 15            # exactly the layers of that map size, not all
    direct = {n.rsplit(".", 1)[0] for n in gone if n.endswith(".wino_in")}
    assert direct <= set(come)                                                   # each of them is a direct launch now


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.change.get("xcd")], ids=lambda c: c.id)
def test_the_xcd_shape_has_grids_the_tile_order_changes(monkeypatch, case):
    """RIB_NO_XCD is read once per process, so the plan cannot show it; the grid figures show that it matters at this shape
    and at none of the smaller ones."""
    assert case.shape == pc.XCD_SHAPE
    assert len(pc.reordered_by_xcd(pc.host_plan(monkeypatch, {}, case.shape).launches)) >= 8
    for shape in pc.SHAPES:
        assert not pc.reordered_by_xcd(pc.host_plan(monkeypatch, {}, shape).launches), shape


def test_every_policy_switch_has_a_row():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "render-in-between_amd", "csrc")
    with open(os.path.join(src, "planner.h")) as f:
        text = f.read()
    policy = text[text.index("struct FusionPolicy {"):text.index("struct Builder {")]
    switches = set(re.findall(r'getenv\("(RIB_[A-Z0-9_]+)"\)', policy)) | {"RIB_NO_XCD"}
    assert len(switches) >= 17 and switches <= set(pc.POLICY_VARS)        # a new switch needs a row, or an A/B test named above
    in_rows = {k for c in pc.CASES for k in list(c.env) + list(c.base)}
    assert switches - HELD_ELSEWHERE == in_rows
    for c in pc.CASES:
        assert c.relation in ("bit", "5e-5", "plan") and c.why and (c.first_tap is not None) == (c.relation == "5e-5"), c.id
