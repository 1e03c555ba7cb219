"""Staged against unstaged Winograd input transforms: the same bits everywhere (run with `-m gpu` on an MI355X).

k_wino_in_staged fetches and modulates every element of a workgroup's input patch once and keeps it in LDS; k_wino_in /
k_wino4_in let every (tile, row) unit fetch its own rows.  Both take the value of an element from wino_fetch / wino_value and
run the transform in the same order, so V - and the joined tensor a lazy join stores - must be bit-identical, and with them
every later launch.  Each side renders on a workspace filled with 0xFF (NaN): an element of V or of a join that a staged
workgroup left unwritten shows.  tests/test_wino_in_staged_cpu.py proves that the two sides differ in at least one `.wino_in`
launch at every shape and setting used here.

The shapes cover maps smaller than a block of tiles (64x64: 2x2 and 4x4 deepest maps), odd maps with partial tiles on both
axes (176x112: 11x7), batch 2, the half-resolution SPADE sources of up_4 / up_3, joins with a second normalised operand and
with a stored residual (`mask.res_*`), and with RIB_WINO_M / RIB_WINO_SHORTCUT_M every (source, second source) pair of both
tile sizes."""
import pytest
import torch

from tests import policy_common as pc

pytestmark = pytest.mark.gpu

ENVS = ({}, {"RIB_WINO_M": "2"}, {"RIB_WINO_M": "4"}, {"RIB_WINO_SHORTCUT_M": "2"}, {"RIB_WINO_SHORTCUT_M": "4"})
FULL = (1, 512, 512)


def env_id(env):
    return "-".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def both_sides(G, fn):
    """fn() with staging on, then off; the handle is left as it was made (on)."""
    try:
        on = fn(G.set_wino_in_staging(True))
        off = fn(G.set_wino_in_staging(False))
    finally:
        G.set_wino_in_staging(True)
    return on, off


def staged_launches(r):
    return [n for n, _, tile in r.launches if tile.startswith("staged")]


@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "%dx%dx%d" % s)      # (the shape varies fastest: one handle per setting)
@pytest.mark.parametrize("env", ENVS, ids=env_id)
def test_staged_transforms_keep_every_bit(monkeypatch, shape, env):
    G = pc.handle(monkeypatch, env)
    on, off = both_sides(G, lambda g: pc.render(g, shape, taps=True))
    assert staged_launches(on) and not staged_launches(off)
    assert [l[0] for l in on.launches] == [l[0] for l in off.launches]
    assert all(bool(torch.isfinite(t).all()) for t in (on.img, on.mask, off.img, off.mask))
    assert on.names == off.names and "mask.res_0" in on.names
    differing = [n for n, a, b in zip(on.names, on.taps, off.taps) if not torch.equal(a, b)]
    assert not differing, ("first differing taps", differing[:6])
    assert torch.equal(on.img, off.img)
    assert torch.equal(on.mask, off.mask)


def test_staged_transforms_keep_every_bit_of_a_chain(monkeypatch):
    shape = pc.SHAPES[1]
    G = pc.handle(monkeypatch, {})
    on, off = both_sides(G, lambda g: [t.clone() for t in pc.render_chain(g, shape)])
    assert len(on) == 3 and all(bool(torch.isfinite(t).all()) for t in on)
    for a, b in zip(on, off):
        assert torch.equal(a, b)


def test_staged_transforms_keep_every_bit_of_the_tuned_512_frame(monkeypatch):
    from render_in_between_amd import synth
    G = pc.handle(monkeypatch, {})
    G.enable_taps(False)
    inputs = [t.cuda() for t in synth.make_inputs(G.spec, *FULL, pc.INPUT_SEED)]      # (no oracle frame at this size: pc.render computes one)

    def render(g):
        staged = [o["name"] for o in g.launch_info(*FULL) if o["tile"].startswith("staged")]
        g._workspace(*FULL).fill_(pc.POISON)
        img, mask = g(inputs[0], None, inputs[1], inputs[2])
        torch.cuda.synchronize()
        return img, mask, staged

    on, off = both_sides(G, render)
    assert len(on[2]) >= 10 and not off[2]
    assert bool(torch.isfinite(on[0]).all()) and bool(torch.isfinite(on[1]).all())
    assert torch.equal(on[0], off[0])
    assert torch.equal(on[1], off[1])
