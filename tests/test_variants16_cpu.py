"""Which 16-bit kernel variants the forced-variant GPU test (tests/test_gpu_variants16.py) reaches.  CPU only: host-only
handles (rib_create(cfg, -1)) build launch plans without a GPU.

The GPU test renders one small frame with a bf16 / half handle, then again with ONE launch pinned to another variant
(rib_set_choice) and compares the debug tap that is that launch's product.  This module holds the case list both tests
use - shape, launches, their taps, split-K factors - and asserts that the list leaves nothing out:

  (a) every k_igemm variant of the precision is accepted by some listed launch,
  (b) so is every (geometry, split-K) pair the measured 16-bit table (tuning_gfx950_bf16.json) pins, at any of its shapes,
  (c) each k_gemm_dma tile is accepted by each condition-level gamma/beta GEMM,
  (d) every tap the GPU test reads exists in the plan.

"Accepted" is what tools/variant_usage.py reads: after rib_set_choice the plan still builds (rib_num_launches > 0) and
the launch's info line names the forced variant and split (a SPADE that is only a modulate of its level's slab builds
a plan too, but runs no kernel of its own: that is not an acceptance)."""
import ctypes as C
import functools
import re

import pytest

import render_in_between_amd as rib
from render_in_between_amd import _native, tuning

B, H, W = SHAPE = (2, 48, 80)      # every map from 48x80 down to 3x5 leaves partial tiles; batch 2: the sample stride
INPUT_SEED = 3                     # synth.make_inputs(spec, 2, 48, 80, 3): the inputs of the two 16-bit frame tests
KSPLITS = (1, 2, 3, 4)             # every factor the 16-bit table names
# launch -> the tap that is its direct product (Builder::spade_block / mask_branch / frame, csrc/planner.h)
LAUNCHES = (
    ("up_4.conv_block_1", "up_4"),                              # 3x3 + its shortcut, deepest map
    ("res_0.conv_block_0", "res_0.h"),
    ("down_1.conv_block_1", "down_1"),                          # 3x3 with the learned 1x1 shortcut fused in
    ("down_0.conv_block_0", "down_0.h"),
    ("up_0.1.spade", "up_0.y1"),                                # fused SPADE, or the unfused pair (1x1 GEMM + modulate)
    ("down_0.0.spade", "down_0.ys0"),                           # two sets
    ("flow_network_temp.down_lbl.0", "mask.lbl_0.raw"),
    ("flow_network_temp.down_lbl.2", "mask.lbl_2.raw"),         # stride 2, InstanceNorm prologue
    ("ref_embedding.down_1", "cond_2"),                         # stride 2, plain
    ("down_first", "down_first"),
    ("flow_network_temp.up_flow.1", "mask.up_0.raw"),           # upsampled gather (phase convolutions)
    ("flow_network_temp.up_flow.3", "mask.up_1.raw"),
    ("flow_network_temp.up_flow.5", "mask.up_2.raw"),
)
GEMM_LEVELS = (1, 2, 3, 4)         # cond_<k>.gammabeta: the level's gamma/beta slab, read by the first SPADE of that level
GEMM_TILES = {"128x64", "64x64", "64x128", "128x128"}
NUM_TAPS = 68                      # taps of the plan of SHAPE: "every earlier tap is bit-equal" is only as long as this list
DTYPES = {"bf16": (1, 1), "f16": (3, 2)}      # name -> (rib_set_compute_dtype code, what rib_variant_info returns)


def gemm_launch(k):
    return "cond_%d.gammabeta" % k


def host_handle(fmt):
    """A host-only handle of the full HSM configuration in the 16-bit mode `fmt`, debug taps on (as the GPU test runs)."""
    lib = _native.lib()
    spec = rib.GenSpec.from_cfg(rib.hsm_gen_config())
    c = _native.RibConfig(**{n: getattr(spec, n) for n, _ in _native.RibConfig._fields_})
    h = C.c_void_p()
    assert lib.rib_create(C.byref(c), -1, C.byref(h)) == 0, lib.rib_last_error(None)
    assert lib.rib_set_compute_dtype(h, DTYPES[fmt][0]) == 0
    assert lib.rib_set_debug_taps(h, 1) == 0
    return lib, h


@functools.lru_cache(maxsize=None)
def variants(fmt):
    """({index: geometry[12]} of the k_igemm variants, {index: "BMxBN"} of the k_gemm_dma tiles) of a precision."""
    lib = _native.lib()
    g = (C.c_int * 12)()
    igemm, tiles = {}, {}
    for i in range(lib.rib_num_variants()):
        if lib.rib_variant_info(i, g) != DTYPES[fmt][1]:
            continue
        if g[0] == 0:                                  # FRW = 0: a k_gemm_dma tile of (32 WM MF) x (32 WN NF)
            tiles[i] = "%dx%d" % (32 * g[1] * g[3], 32 * g[2] * g[4])
        else:
            igemm[i] = tuple(g)
    return igemm, tiles


def launch_lines(lib, h):
    """{launch name: its rib_debug_launch_info line} of the plan of SHAPE, or None where no plan can be built."""
    n = lib.rib_num_launches(h, B, H, W)
    if n <= 0:
        return None
    buf = C.create_string_buffer(512)
    out = {}
    for i in range(n):
        assert lib.rib_debug_launch_info(h, B, H, W, i, buf, 512) == 0
        line = buf.value.decode()
        out[line.split("|", 1)[0]] = line
    return out


def tap_list(lib, h):
    """[(name, C, H, W)] of the plan's taps, in plan order."""
    name = C.c_char_p(); ch = C.c_int(); th = C.c_int(); tw = C.c_int()
    out = []
    for i in range(lib.rib_num_taps(h, B, H, W)):
        assert lib.rib_tap_info(h, B, H, W, i, C.byref(name), C.byref(ch), C.byref(th), C.byref(tw)) == 0
        out.append((name.value.decode(), ch.value, th.value, tw.value))
    return out


def gemm_tap(taps, k):
    """The tap that reads cond_<k>.gammabeta's slab first: the first `.ys0` in plan order on a map of cond_<k>'s size (there
    the gamma/beta are fp32 and the modulate is elementwise, so the tap carries one rounding of the GEMM's product)."""
    size = {n: (th, tw) for n, _, th, tw in taps}["cond_%d" % k]
    return next(n for n, _, th, tw in taps if n.endswith(".ys0") and (th, tw) == size)


def gemm_taps(taps, k):
    """Every SPADE output tap (`.ys0`, `.y1`) on a map of cond_<k>'s size, in plan order: the tapped readers of the level's slab,
    gemm_tap(taps, k) first."""
    size = {n: (th, tw) for n, _, th, tw in taps}["cond_%d" % k]
    return [n for n, _, th, tw in taps if n.endswith((".ys0", ".y1")) and (th, tw) == size]


def takes_choice(lib, h, fmt, launch, vi, ks):
    """Pins (variant, ksplit) on `launch`: does the plan of SHAPE still build, and does the launch's line name that choice?
    The choice stays pinned (the caller renders with it, or erases it with variant -1)."""
    assert lib.rib_set_choice(h, B, H, W, launch.encode(), vi, ks) == 0
    if lib.rib_workspace_bytes(h, B, H, W) == 0:
        return False                                   # the plan builder refuses: does not fit this launch
    line = launch_lines(lib, h).get(launch, "")
    tile = variants(fmt)[1].get(vi)
    if tile is not None:
        return ks == 1 and ("gemm (LDS-DMA staged operands) tile %s " % tile) in line
    return re.search(r" ksplit%d .* v%d\|" % (ks, vi), line) is not None


def candidates(fmt, launch):
    """Every (variant of the precision, ksplit) the tests try on `launch`: the GEMM tiles on a gamma/beta GEMM, else k_igemm."""
    igemm, tiles = variants(fmt)
    return [(vi, 1) for vi in tiles] if launch.endswith(".gammabeta") else [(vi, ks) for vi in igemm for ks in KSPLITS]


@functools.lru_cache(maxsize=None)
def accepted(fmt, launch):
    """((variant index, ksplit), ...) that the plan builder accepts for `launch` at SHAPE, in the order the GPU test tries them."""
    lib, h = host_handle(fmt)
    try:
        out = tuple(c for c in candidates(fmt, launch) if takes_choice(lib, h, fmt, launch, *c))
        assert lib.rib_set_choice(h, B, H, W, launch.encode(), -1, 1) == 0
    finally:
        lib.rib_destroy(h)
    return out


def table_pairs():
    """({(geometry[12], ksplit)} of the k_igemm entries, {"BMxBN"} of the GEMM tiles) that the 16-bit table pins, over all
    its shapes (an entry: geometry[10] + [ksplit] (+ [KW, TB]), tuning.apply)."""
    pairs, tiles = set(), set()
    for entry in tuning.load(dtype="bf16").values():
        for choice in entry.values():
            kw = int(choice[11]) if len(choice) > 11 else 1
            tb = int(choice[12]) if len(choice) > 12 else 1
            g = tuple(int(v) for v in choice[:10]) + (kw, tb)
            if g[0] == 0:
                tiles.add("%dx%d" % (32 * g[1] * g[3], 32 * g[2] * g[4]))
            else:
                pairs.add((g, int(choice[10])))
    return pairs, tiles


@pytest.mark.parametrize("fmt", sorted(DTYPES))
def test_forced_variant_cases_reach_every_16_bit_kernel(fmt):
    igemm, tiles = variants(fmt)
    assert len(igemm) == 45 and set(tiles.values()) == GEMM_TILES, (len(igemm), tiles)
    acc = {name: accepted(fmt, name) for name, _ in LAUNCHES}
    # every listed launch takes part
    assert all(acc.values()), [n for n, a in acc.items() if not a]
    # (a) every k_igemm variant of the precision runs on some listed launch
    reached = {vi for a in acc.values() for vi, _ in a}
    assert reached == set(igemm), sorted(igemm[v] for v in set(igemm) - reached)
    # (b) every (geometry, split-K) pair of the measured table, at whichever shape it is pinned
    pairs, table_tiles = table_pairs()
    assert len(pairs) >= 40 and table_tiles, (len(pairs), table_tiles)
    have = {(igemm[vi], ks) for a in acc.values() for vi, ks in a}
    assert pairs <= have, sorted(pairs - have)
    assert {ks for _, ks in pairs} <= set(KSPLITS)
    # (c) every GEMM tile on every condition-level GEMM (the table's tiles among them)
    for k in GEMM_LEVELS:
        got = accepted(fmt, gemm_launch(k))
        assert {tiles[vi] for vi, _ in got} == GEMM_TILES, (k, got)
    assert table_tiles <= GEMM_TILES
    # (d) every tap the GPU test reads exists, and the gamma/beta slabs have a reader that is a tap
    lib, h = host_handle(fmt)
    try:
        taps = tap_list(lib, h)
        names = [n for n, _, _, _ in taps]
        assert len(set(names)) == len(names) == NUM_TAPS
        for _, tap in LAUNCHES:
            assert tap in names, tap
        assert [gemm_tap(taps, k) for k in GEMM_LEVELS] == ["down_%d.ys0" % k for k in GEMM_LEVELS]
        for k in GEMM_LEVELS:      # the level's tapped SPADE outputs: both of down_k and of up_k (level 4: the res blocks' too)
            assert gemm_taps(taps, k)[0] == gemm_tap(taps, k) and len(gemm_taps(taps, k)) >= 4, gemm_taps(taps, k)
    finally:
        lib.rib_destroy(h)
