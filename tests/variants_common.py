"""What the forced-variant tests of every precision share (tests/test_variants16_cpu.py, tests/test_variants32_cpu.py and
their GPU files): the shape, and the helpers that pin ONE launch of its plan to another kernel variant (rib_set_choice)
and read back whether the plan builder took it.  Host-only handles (rib_create(cfg, -1)) build launch plans without a
GPU; every helper here works on those and on a Generator's handle alike.

"Accepted" is what tools/variant_usage.py reads: after rib_set_choice the plan still builds (rib_num_launches > 0) and
the launch's info line names the forced variant and split, or the forced GEMM tile (a SPADE that is only a modulate of
its level's slab builds a plan too, but runs no kernel of its own: that is not an acceptance)."""
import ctypes as C
import functools
import re

import render_in_between_amd as rib
from render_in_between_amd import _native, tuning

B, H, W = SHAPE = (2, 48, 80)      # every map from 48x80 down to 3x5 leaves partial tiles; batch 2: the sample stride
INPUT_SEED = 3                     # synth.make_inputs(spec, 2, 48, 80, 3)
NUM_TAPS = 68                      # taps of the plan of SHAPE: "every earlier tap is bit-equal" is only as long as this list
PREC = {"f32": (0, 0), "bf16": (1, 1), "f16": (3, 2)}      # name -> (rib_set_compute_dtype code, what rib_variant_info returns)


def host_handle(fmt):
    """A host-only handle of the full HSM configuration in the precision mode `fmt`, debug taps on (as the GPU tests run);
    no measured table is applied to it (what use_tuning=False gives a Generator)."""
    lib = _native.lib()
    spec = rib.GenSpec.from_cfg(rib.hsm_gen_config())
    c = _native.RibConfig(**{n: getattr(spec, n) for n, _ in _native.RibConfig._fields_})
    h = C.c_void_p()
    assert lib.rib_create(C.byref(c), -1, C.byref(h)) == 0, lib.rib_last_error(None)
    assert lib.rib_set_compute_dtype(h, PREC[fmt][0]) == 0
    assert lib.rib_set_debug_taps(h, 1) == 0
    return lib, h


@functools.lru_cache(maxsize=None)
def variants(fmt):
    """({index: geometry[12]} of the k_igemm variants, {index: "BMxBN"} of the k_gemm_dma tiles) of a precision."""
    lib = _native.lib()
    g = (C.c_int * 12)()
    igemm, tiles = {}, {}
    for i in range(lib.rib_num_variants()):
        if lib.rib_variant_info(i, g) != PREC[fmt][1]:
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


def gemm_launch(k):
    return "cond_%d.gammabeta" % k


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


def accepted_of(fmt, launch, cands):
    """((variant index, ksplit), ...) of `cands` that the plan builder accepts for `launch` at SHAPE, in their order."""
    lib, h = host_handle(fmt)
    try:
        out = tuple(c for c in cands if takes_choice(lib, h, fmt, launch, *c))
        assert lib.rib_set_choice(h, B, H, W, launch.encode(), -1, 1) == 0
    finally:
        lib.rib_destroy(h)
    return out


def table_pairs(dtype):
    """({(geometry[12], ksplit)} of the k_igemm entries, {"BMxBN"} of the GEMM tiles) that the measured table of `dtype` pins,
    over all its shapes (an entry: geometry[10] + [ksplit] (+ [KW, TB]), tuning.apply)."""
    pairs, tiles = set(), set()
    for entry in tuning.load(dtype=dtype).values():
        for choice in entry.values():
            kw = int(choice[11]) if len(choice) > 11 else 1
            tb = int(choice[12]) if len(choice) > 12 else 1
            g = tuple(int(v) for v in choice[:10]) + (kw, tb)
            if g[0] == 0:
                tiles.add("%dx%d" % (32 * g[1] * g[3], 32 * g[2] * g[4]))
            else:
                pairs.add((g, int(choice[10])))
    return pairs, tiles
