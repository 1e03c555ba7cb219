"""Staged Winograd input transforms (k_wino_in_staged, rib_set_wino_in_staging): what the switch may and may not change in a
launch plan, on host-only handles.

Both sides of the switch must run the same launches in the same order on the same workspace with the same taps; only the
(grid, tile) of `.wino_in` launches may differ, and at every shape and Winograd setting at least one must differ - otherwise
the GPU comparison of the two sides (tests/test_gpu_wino_in_staged.py) would compare a plan with itself."""
import ctypes as C

import pytest

import render_in_between_amd as rib
from tests import policy_common as pc
from render_in_between_amd import _native

SHAPES = pc.SHAPES + ((1, 512, 512),)
ENVS = ({}, {"RIB_WINO_M": "2"}, {"RIB_WINO_M": "4"}, {"RIB_WINO_SHORTCUT_M": "2"}, {"RIB_WINO_SHORTCUT_M": "4"})
OFF_VAR = "RIB_WINO_IN_UNSTAGED"


def env_id(env):
    return "-".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def plan(monkeypatch, env, shape, staged, taps=True):
    """The host plan of `shape` under `env` with the staging switch in the given position (read by rib_create)."""
    monkeypatch.delenv(OFF_VAR, raising=False)
    return pc.host_plan(monkeypatch, env if staged else dict(env, **{OFF_VAR: "1"}), shape, taps=taps)


@pytest.mark.parametrize("env", ENVS, ids=env_id)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_switch_changes_wino_in_grids_and_nothing_else(monkeypatch, shape, env):
    on, off = plan(monkeypatch, env, shape, True), plan(monkeypatch, env, shape, False)
    assert [l[0] for l in on.launches] == [l[0] for l in off.launches]
    assert on.ws_bytes == off.ws_bytes
    assert on.taps == off.taps
    differ = [a[0] for a, b in zip(on.launches, off.launches) if a != b]
    assert differ, "no launch is staged at %s under %s" % (shape, env)
    assert all(n.endswith(".wino_in") for n in differ), differ
    # the unstaged side names no block of tiles; a staged launch does
    assert not any(l[2].startswith("staged") for l in off.launches)
    assert all(l[2].startswith("staged") for l in on.launches if l[0] in differ)


def test_the_plans_without_taps_differ_in_the_same_way(monkeypatch):
    on, off = plan(monkeypatch, {}, (1, 512, 512), True, taps=False), plan(monkeypatch, {}, (1, 512, 512), False, taps=False)
    assert [l[0] for l in on.launches] == [l[0] for l in off.launches] and on.ws_bytes == off.ws_bytes
    differ = [a[0] for a, b in zip(on.launches, off.launches) if a != b]
    assert differ and all(n.endswith(".wino_in") for n in differ)


def test_the_setter_rebuilds_the_plans(monkeypatch):
    """rib_set_wino_in_staging on a live handle gives the plan the environment default gives a new one, in both directions."""
    shape = (1, 176, 112)
    want = {s: plan(monkeypatch, {}, shape, s, taps=False).launches for s in (True, False)}
    monkeypatch.delenv(OFF_VAR, raising=False)
    lib = _native.lib()
    spec = rib.GenSpec.from_cfg(rib.hsm_gen_config())
    c = _native.RibConfig(**{n: getattr(spec, n) for n, _ in _native.RibConfig._fields_})
    h = C.c_void_p()
    assert lib.rib_create(C.byref(c), -1, C.byref(h)) == 0

    def launches():
        buf = C.create_string_buffer(600)
        out = []
        for i in range(lib.rib_num_launches(h, *shape)):
            assert lib.rib_debug_launch_info(h, *shape, i, buf, 600) == 0
            name, _, grid, tile, _, _ = buf.value.decode().split("|")
            out.append((name, grid, tile))
        return out

    try:
        assert launches() == want[True]
        for staged in (False, True, True, False):
            assert lib.rib_set_wino_in_staging(h, 1 if staged else 0) == 0
            assert launches() == want[staged]
        assert lib.rib_set_wino_in_staging(None, 1) != 0
    finally:
        lib.rib_destroy(h)
