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
a plan too, but runs no kernel of its own: that is not an acceptance).  The helpers are tests/variants_common.py's, which
the fp32 files (tests/test_variants32_cpu.py, tests/test_gpu_variants32.py) use too."""
import functools

import pytest

from tests.variants_common import (B, H, INPUT_SEED, NUM_TAPS, PREC, SHAPE, W, accepted_of, gemm_launch, gemm_tap,      # noqa: F401
                                   gemm_taps, host_handle, launch_lines, tap_list, takes_choice, variants)               # (the GPU file's too)
from tests import variants_common

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
DTYPES = {fmt: PREC[fmt] for fmt in ("bf16", "f16")}


def candidates(fmt, launch):
    """Every (variant of the precision, ksplit) the tests try on `launch`: the GEMM tiles on a gamma/beta GEMM, else k_igemm."""
    igemm, tiles = variants(fmt)
    return [(vi, 1) for vi in tiles] if launch.endswith(".gammabeta") else [(vi, ks) for vi in igemm for ks in KSPLITS]


@functools.lru_cache(maxsize=None)
def accepted(fmt, launch):
    """((variant index, ksplit), ...) that the plan builder accepts for `launch` at SHAPE, in the order the GPU test tries them."""
    return accepted_of(fmt, launch, candidates(fmt, launch))


def table_pairs():
    """The (geometry, split-K) pairs and the GEMM tiles that the 16-bit table (tuning_gfx950_bf16.json) pins."""
    return variants_common.table_pairs("bf16")


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
