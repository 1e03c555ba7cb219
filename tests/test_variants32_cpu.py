"""Which fp32 kernel variants the forced-variant GPU test (tests/test_gpu_variants32.py) reaches.  CPU only: host-only
handles (rib_create(cfg, -1)) build launch plans without a GPU.

The fp32 counterpart of tests/test_variants16_cpu.py.  The GPU test renders one 2x48x80 frame with an fp32 handle
(use_tuning=False, debug taps on), then again with ONE launch pinned to another variant (rib_set_choice) and compares
the debug tap that is that launch's product with the default plan's and with the fp64 oracle's.  This module holds the
case list both tests use - shape, launches, their taps, split-K factors - and asserts that the list leaves nothing out:

  (a) every fp32 k_igemm variant is accepted by some listed launch,
  (b) so is every (geometry, split-K) pair the measured fp32 table (tuning_gfx950.json) pins, at any of its shapes,
  (c) each fp32 k_gemm_dma tile is accepted by each listed GEMM (the condition levels' gamma/beta GEMMs and three
      Winograd position GEMMs of different M),
  (d) every tap the GPU test reads exists in the plan, once.

All four are set equalities or inclusions: a variant, a table pair or a tile that a later change adds and no listed
launch takes fails this file by name.  "Accepted" and the helpers are tests/variants_common.py's."""
import functools

from tests.variants_common import (B, H, INPUT_SEED, NUM_TAPS, SHAPE, W, accepted_of, gemm_launch, gemm_tap,      # noqa: F401
                                   host_handle, launch_lines, table_pairs, tap_list, takes_choice, variants)      # (the GPU file's too)

FMT = "f32"
KSPLITS = (1, 2, 3, 4, 8)          # every factor the fp32 table names
# launch -> the tap that is its direct product (Builder::spade_block / mask_branch / frame, csrc/planner.h).  The first seven
# reach every variant and every table pair between them (without 8 in KSPLITS, or with any of the seven but
# down_3.conv_block_0 taken out of them, (a) or (b) fails by name; that one is the 16-column 3x3 tiles' small map); the
# other eight give every kernel family a second map size.
LAUNCHES = (
    ("down_3.conv_block_0", "down_3.h"),                        # 3x3 on a 6x10 map: the 16-column tiles
    ("ref_embedding.down_2", "cond_3"),                         # stride 2, plain
    ("down_0.1.spade", "down_0.y1"),                            # fused SPADE, or the unfused pair (1x1 GEMM + modulate)
    ("flow_network_temp.up_flow.1", "mask.up_0.raw"),           # upsampled gather (phase convolutions)
    ("up_0.conv_block_0", "up_0.h"),                            # 3x3 on the full-size map
    ("down_4.conv_block_1", "down_4"),                          # 3x3 with the learned 1x1 shortcut fused in, deepest map
    # a 1x1 shortcut of the mask network.  mask.res_0 is the first tap behind it, not its bare product: the shortcut is
    # summed with conv_block_1's output there (both in fp32, elementwise)
    ("flow_network_temp.res_flow.0.conv_block_s", "mask.res_0"),
    ("down_1.conv_block_1", "down_1"),
    ("up_2.conv_block_0", "up_2.h"),
    ("up_4.conv_block_1", "up_4"),
    ("down_0.0.spade", "down_0.ys0"),                           # two sets
    ("flow_network_temp.down_lbl.2", "mask.lbl_2.raw"),         # stride 2, InstanceNorm prologue
    ("flow_network_temp.down_img.1", "mask.img_1.raw"),
    ("flow_network_temp.up_flow.5", "mask.up_2.raw"),
    ("ref_embedding.down_0", "cond_1"),
)
# A choice name that a second launch follows.  Level i >= 1 of the mask network's two encoders is the same convolution on
# other tensors, and both take the choice named after the image encoder's (Builder::mask_branch: the kernel of the paired
# launch of batch-1 plans), so pinning down_img.1 pins down_lbl.1 as well: launch -> (the follower, its product tap, the
# taps ahead of `launch`'s own that are computed from that product).  The follower's product is held like the launch's own.
FOLLOWERS = {"flow_network_temp.down_img.1": ("flow_network_temp.down_lbl.1", "mask.lbl_1.raw", ("mask.lbl_2.raw",))}
GEMM_LEVELS = (1, 2, 3, 4)         # cond_<k>.gammabeta: the level's gamma/beta slab; its tap is gemm_tap(taps, k)
# Winograd position GEMMs (16 or 36 GEMMs of M = tiles of the map) -> the first tap behind their output transform
WINO_GEMMS = (
    ("down_4.conv_block_0.wino", "down_4.h"),
    ("up_3.conv_block_0.wino", "up_3.h"),
    ("flow_network_temp.res_flow.0.conv_block_0.wino", "mask.res_0"),
)
GEMM_TILES = {"128x64", "64x64", "64x128", "128x128", "128x32"}


def gemms(taps):
    """((launch, first tap behind it), ...) of the k_gemm_dma launches the tests force; taps: tap_list of the plan."""
    return tuple((gemm_launch(k), gemm_tap(taps, k)) for k in GEMM_LEVELS) + WINO_GEMMS


def candidates(launch):
    """Every (fp32 variant, ksplit) the tests try on `launch`: the GEMM tiles on a k_gemm_dma launch, else k_igemm x KSPLITS."""
    igemm, tiles = variants(FMT)
    if launch.endswith((".gammabeta", ".wino")):
        return [(vi, 1) for vi in tiles]
    return [(vi, ks) for vi in igemm for ks in KSPLITS]


@functools.lru_cache(maxsize=None)
def accepted(launch):
    """((variant index, ksplit), ...) that the plan builder accepts for `launch` at SHAPE, in the order the GPU test tries them."""
    return accepted_of(FMT, launch, candidates(launch))


def unreached(launches):
    """(fp32 k_igemm variants, (geometry, split-K) pairs of the measured table) that none of `launches` accepts."""
    igemm, _ = variants(FMT)
    acc = [accepted(name) for name in launches]
    pairs, _ = table_pairs(FMT)
    return (sorted((v, g) for v, g in igemm.items() if v not in {vi for a in acc for vi, _ in a}),
            sorted(pairs - {(igemm[vi], ks) for a in acc for vi, ks in a}))


def test_forced_variant_cases_reach_every_fp32_kernel():
    igemm, tiles = variants(FMT)
    assert igemm and set(tiles.values()) == GEMM_TILES and len(tiles) == len(GEMM_TILES), (len(igemm), tiles)
    # every listed launch takes part
    assert all(accepted(name) for name, _ in LAUNCHES), [n for n, _ in LAUNCHES if not accepted(n)]
    # the table speaks of this library's kernels, and of every factor the tests try
    pairs, table_tiles = table_pairs(FMT)
    assert pairs and {g for g, _ in pairs} <= set(igemm.values()), sorted({g for g, _ in pairs} - set(igemm.values()))
    assert {ks for _, ks in pairs} == set(KSPLITS)
    assert table_tiles <= GEMM_TILES
    # (a) every fp32 k_igemm variant runs on some listed launch; (b) so does every (geometry, split-K) pair of the measured
    # table, at whichever shape it is pinned.  The first seven launches do that by themselves.
    assert unreached([name for name, _ in LAUNCHES]) == ([], [])
    assert unreached([name for name, _ in LAUNCHES[:7]]) == ([], [])
    # (c), (d) on the plan's own tap list
    lib, h = host_handle(FMT)
    try:
        taps = tap_list(lib, h)
        lines = launch_lines(lib, h)
    finally:
        lib.rib_destroy(h)
    names = [n for n, _, _, _ in taps]
    assert len(set(names)) == len(names) == NUM_TAPS
    # (c) every GEMM tile on every listed GEMM (the table's tiles among them)
    for launch, tap in gemms(taps):
        got = accepted(launch)
        assert {tiles[vi] for vi, _ in got} == GEMM_TILES and len(got) == len(GEMM_TILES), (launch, got)
        assert tap in names, tap
    assert [gemm_tap(taps, k) for k in GEMM_LEVELS] == ["down_%d.ys0" % k for k in GEMM_LEVELS]
    # (d) every tap the GPU test reads exists; every launch it pins is in the default plan, once in either list
    for launch, tap in LAUNCHES:
        assert tap in names and launch in lines, (launch, tap)
    for launch, (follower, ftap, behind) in FOLLOWERS.items():
        tap = dict(LAUNCHES)[launch]
        assert follower in lines and names.index(ftap) < min(names.index(t) for t in behind + (tap,)), (launch, follower)
    pinned = [l for l, _ in LAUNCHES + gemms(taps)]
    assert len(set(pinned)) == len(pinned)
    assert len({t for _, t in LAUNCHES}) == len(LAUNCHES)


def test_a_pinned_choice_moves_the_launches_it_names_and_no_other():
    """What "every tap ahead of the product tap is bit-equal" rests on: with a listed launch pinned, the only lines of the
    plan that name another kernel variant or split than the default plan's are that launch's, its follower's (FOLLOWERS:
    the same variant and split as the launch itself) and launches that the pinned one adds or drops (a split's slab sum,
    the modulate of an unfused SPADE)."""
    kernel = lambda line: line.split("|")[3]           # the tile / variant text of a rib_debug_launch_info line
    lib, h = host_handle(FMT)
    try:
        base = launch_lines(lib, h)
        for launch, _ in LAUNCHES:
            follower = FOLLOWERS.get(launch, (None,))[0]
            for vi, ks in accepted(launch):
                assert takes_choice(lib, h, FMT, launch, vi, ks)
                lines = launch_lines(lib, h)
                moved = {n for n in set(base) & set(lines) if kernel(base[n]) != kernel(lines[n])} - {launch}
                assert moved <= ({follower} if follower else set()), (launch, vi, ks, sorted(moved))
                if follower:
                    assert kernel(lines[follower]) == kernel(lines[launch]), (lines[follower], lines[launch])
            assert lib.rib_set_choice(h, B, H, W, launch.encode(), -1, 1) == 0
    finally:
        lib.rib_destroy(h)
