"""What tests/test_policy_cpu.py and tests/test_gpu_policy.py share: the table of launch-plan policy switches and the helpers
that build a plan, or render a frame, on each side of one.

Every switch of `struct FusionPolicy` (csrc/planner.h) and the ones read elsewhere (RIB_NO_XCD, RIB_NO_PAIR) gives two
implementations of the same frame from the same inputs.  A row of CASES names the switch setting, the shape, the relation the
two frames must satisfy and what the setting changes in the launch list.  The CPU file proves on host-only handles that
every row changes the plan in the way it names (no GPU case is vacuous); the GPU file renders both sides on workspaces
filled with 0xFF and holds them to the relation:

  "bit"    the two sides perform the same arithmetic on every element: torch.equal on both outputs and on every tap
  "5e-5"   a summation order or a kernel family changes: frames within 5e-5 of the default plan's (the bar of the other
           "same layer, another summation order" tests), both within 2e-4 of the oracle; with taps on every tap ahead of
           `first_tap` bit-equal, first_tap within 5e-5 * max(1, max|ref|), later taps within 2e-4 * max(1, max|ref|)
  "plan"   asserted on the launch list only (the arithmetic of the two sides has a GPU test of its own, named in `why`)

The bars are the suite's; none is derived from what the kernels give."""
import collections
import ctypes as C
import os
import re
import sys

import render_in_between_amd as rib
from render_in_between_amd import _native

SHAPES = ((1, 64, 64), (2, 48, 80), (1, 176, 112))      # 176x112: 11x7 deepest maps, partial tiles everywhere
XCD_SHAPE = (1, 128, 128)                                # the smallest of the suite's usual shapes with grids xcd_chunk_of reorders
CHAIN_T = 3
TOL_AB = 5e-5
TOL_ORACLE = 2e-4
INPUT_SEED = 11

# every environment switch that shapes a launch plan: cleared before a side is built, so that a side is exactly its row
POLICY_VARS = ("RIB_NO_CONSUMER_STATS", "RIB_NO_SPLITK", "RIB_NO_N16", "RIB_NO_UNFUSED_SPADE", "RIB_NO_LAZY", "RIB_NO_FUSE_SHORTCUT",
               "RIB_NO_WS_REUSE", "RIB_NO_PAIR", "RIB_NO_XCD", "RIB_NO_DMA", "RIB_COND_GEMM_MAX_PX", "RIB_WINO_MAX_PX", "RIB_NO_WINO",
               "RIB_WINO_M", "RIB_NO_LOWC", "RIB_LOWC_TW", "RIB_NO_HEADCONV", "RIB_NO_SMALLCONV", "RIB_NO_LABEL_BATCH", "RIB_NO_SPADE16",
               "RIB_NO_WINO_SHORTCUT", "RIB_WINO_SHORTCUT_M", "RIB_GRAPH")

# id: unique; env: the switched side; base: the side it is compared with ({}: the default plan); shape: (B, H, W);
# relation: "bit" / "5e-5" / "plan"; first_tap: the tap at which a difference may begin (5e-5 rows); change: how the launch
# list differs, checked by test_policy_cpu.py (see check_change there); ignore: launches left out when first_tap is derived;
# why: one line on the relation
Case = collections.namedtuple("Case", "id env base shape relation first_tap change ignore why")


def _rows(name, env, relation, why, change, first_taps=None, shapes=SHAPES, base=None, ignore=()):
    return [Case("%s-%dx%dx%d" % ((name,) + s), dict(env), dict(base or {}), s, relation, (first_taps or {}).get(s), dict(change), ignore, why)
            for s in shapes]


COND0 = {"RIB_COND_GEMM_MAX_PX": "0"}
CASES = (
    # ---- the two sides perform the same arithmetic ------------------------------------------------------------------------
    _rows("ws_reuse", {"RIB_NO_WS_REUSE": "1"}, "bit", "addresses only: every launch and every operand value is the same",
          {"same": True, "ws_larger": True})
    + _rows("lazy", {"RIB_NO_LAZY": "1"}, "bit",
            "a lazy SPADE source is spade_mod1 in the input transform, the stored one spade_mod1 in k_spade_modulate; a lazy join is "
            "k_in_add's expression in the transform: the same fp32 operations on the same operands",
            {"come": (".spade.modulate", ".join"), "n_come": 7})
    + _rows("pair", {"RIB_NO_PAIR": "1"}, "bit",
            "a paired launch is the two single launches side by side in one grid: same kernel, same choice, same K order per sample",
            {"come": ("down_lbl.", "down_img."), "gone": ("down_pair.",), "n_come": 12, "n_gone": 6}, shapes=(SHAPES[0], SHAPES[2]))
    + _rows("pair_b2", {"RIB_NO_PAIR": "1"}, "plan", "nothing is paired at batch 2: the switch must not touch the plan", {"same": True},
            shapes=(SHAPES[1],))
    + _rows("xcd", {"RIB_NO_XCD": "1"}, "bit",
            "the order in which workgroups take tiles only: every tile is computed by the same code from the same operands "
            "(read once per process: the switched side renders in a child process)", {"xcd": True}, shapes=(XCD_SHAPE,))
    # ---- a summation order or a kernel family changes ---------------------------------------------------------------------
    + _rows("consumer_stats", {"RIB_NO_CONSUMER_STATS": "1"}, "5e-5",
            "a consumer adds the fp64 partials in 4 slices (block_stats_64), k_stats_finalize in 64 or 256 and a shuffle tree: the "
            "same terms in another association, so (scale, shift) may differ in the last fp32 bit",
            {"come": (".stats",), "min_come": 26, "max_come": 30},
            {SHAPES[0]: "down_2.ys0", SHAPES[1]: "down_0.y1", SHAPES[2]: "down_1.ys0"})
    + _rows("splitk", {"RIB_NO_SPLITK": "1"}, "5e-5", "K summed in one accumulator instead of ksplit partial sums added afterwards",
            {"gone": (".splitk_sum",), "min_gone": 17, "max_gone": 18, "retile_gone_bases": "ksplit1 "},
            {SHAPES[0]: "cond_1", SHAPES[1]: "cond_1", SHAPES[2]: "cond_2"})
    + _rows("n16", {"RIB_NO_N16": "1"}, "5e-5", "16-column MFMA (16x16x4) against the 32-column one (32x32x2): another K grouping per step",
            {"retile": 1}, {s: "up_0.h" for s in SHAPES})
    + _rows("fuse_shortcut", {"RIB_NO_FUSE_SHORTCUT": "1"}, "5e-5",
            "the 1x1 shortcut as extra K chunks of conv_block_1's accumulator against a launch of its own whose rounded result is added",
            {"come": (".conv_block_s",), "n_come": 13}, {s: "down_0" for s in SHAPES})
    + _rows("cond_gemm", COND0, "5e-5", "gamma/beta from one k_gemm_dma per level against one 1x1 k_igemm (split-K on small maps) per SPADE",
            {"gone": (".gammabeta",), "come": (".spade",), "min_come": 20, "max_come": 28},
            {SHAPES[0]: "down_0.ys0", SHAPES[1]: "down_1.ys0", SHAPES[2]: "down_2.ys0"},
            ignore=(".gammabeta",))      # a level GEMM writes a slab only; its first reader is the level's first SPADE
    + _rows("cond_gemm_fused_spade", dict(COND0, RIB_NO_UNFUSED_SPADE="1"), "5e-5",
            "as cond_gemm, and the small maps' SPADEs modulate in k_igemm<SPADE>'s epilogue from the fp32 accumulators instead of a slab",
            {"gone": (".gammabeta", ".spade.modulate"), "gone_may": (".stats",), "come": (".spade",), "min_come": 16, "max_come": 24},
            {SHAPES[0]: "down_0.ys0", SHAPES[1]: "down_1.ys0", SHAPES[2]: "down_2.ys0"}, ignore=(".gammabeta",))
    # ---- plan only ----------------------------------------------------------------------------------------------------------
    + _rows("unfused_spade_alone", {"RIB_NO_UNFUSED_SPADE": "1"}, "plan",
            "its threshold (pixels x batch <= 4096) is the level GEMM's, and a SPADE served by a level slab is unfused regardless: a "
            "no-op alone at these shapes", {"same": True})
    + _rows("unfused_spade", dict(COND0, RIB_NO_UNFUSED_SPADE="1"), "plan",
            "against RIB_COND_GEMM_MAX_PX=0 alone: the pairs (1x1 GEMM + modulate) become k_igemm<SPADE> launches; the frame is held by "
            "cond_gemm_fused_spade", {"gone": (".spade.modulate",), "gone_may": (".stats",), "min_gone": 12, "retile_gone_bases": ""}, base=COND0)
    + _rows("wino_max_px", {"RIB_WINO_MAX_PX": "largest"}, "plan",
            "the threshold is inclusive; Winograd against direct arithmetic is test_winograd_path_agrees_with_the_direct_convolutions",
            {"wino_threshold": True})
)
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)


def cases(*relations):
    return [c for c in CASES if c.relation in relations]


def clean_env(monkeypatch, env=()):
    """The process environment with every plan switch cleared, then `env` set."""
    for k in POLICY_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)


# ---- host-only plans ----------------------------------------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "launches ws_bytes taps")      # launches: [(name, grid, tile)]; taps: [(name, C, H, W)]


def host_plan(monkeypatch, env, shape, taps=False):
    """The launch plan of `shape` under `env` on a host-only handle (rib_create(cfg, -1)) of the full configuration."""
    clean_env(monkeypatch, env)
    lib = _native.lib()
    B, H, W = shape
    spec = rib.GenSpec.from_cfg(rib.hsm_gen_config())
    c = _native.RibConfig(**{n: getattr(spec, n) for n, _ in _native.RibConfig._fields_})
    h = C.c_void_p()
    assert lib.rib_create(C.byref(c), -1, C.byref(h)) == 0, lib.rib_last_error(None)
    try:
        if taps:
            assert lib.rib_set_debug_taps(h, 1) == 0
        n = lib.rib_num_launches(h, B, H, W)
        assert n > 0, lib.rib_last_error(h)
        buf = C.create_string_buffer(600)
        launches = []
        for i in range(n):
            assert lib.rib_debug_launch_info(h, B, H, W, i, buf, 600) == 0
            name, _, grid, tile, _, _ = buf.value.decode().split("|")
            launches.append((name, grid, tile))
        ws = lib.rib_workspace_bytes(h, B, H, W)
        name = C.c_char_p(); ch = C.c_int(); th = C.c_int(); tw = C.c_int()
        tl = []
        for i in range(lib.rib_num_taps(h, B, H, W)):
            assert lib.rib_tap_info(h, B, H, W, i, C.byref(name), C.byref(ch), C.byref(th), C.byref(tw)) == 0
            tl.append((name.value.decode(), ch.value, th.value, tw.value))
    finally:
        lib.rib_destroy(h)
    return Plan(launches, ws, tl)


def diff(base, other):
    """(names only in `other`, names only in `base`, names in both whose grid or tile differs), each in plan order."""
    bn, on = {l[0]: l for l in base}, {l[0]: l for l in other}
    return ([n for n, _, _ in other if n not in bn], [n for n, _, _ in base if n not in on],
            [n for n, _, _ in base if n in on and on[n] != bn[n]])


MASK_DOWN = 3      # levels of the mask network's encoders below the first (HSM configuration): the last lands in mask.cat.raw


def tap_of_launch(name):
    """The debug tap a launch writes (Builder::spade_block / mask_branch / frame, csrc/planner.h), or None: a launch that writes
    statistics arrays, a gamma/beta slab, a pooled map or a caller's tensor."""
    if name.endswith(".stats") or name.endswith(".gammabeta"):
        return None
    m = re.match(r"ref_embedding\.(conv_first|down_(\d+))", name)
    if m:
        return "cond_0" if m.group(2) is None else "cond_%d" % (int(m.group(2)) + 1)
    if name.startswith("down_first"):
        return "down_first"
    m = re.match(r"((?:down|up|res)_\d+)\.(0\.spade|1\.spade|conv_block_0|conv_block_1|conv_block_s)", name)
    if m:
        return m.group(1) + {"0.spade": ".ys0", "1.spade": ".y1", "conv_block_0": ".h", "conv_block_1": "", "conv_block_s": ""}[m.group(2)]
    m = re.match(r"flow_network_temp\.down_(lbl|img|pair)\.(\d+)", name)
    if m:
        i = int(m.group(2))
        return "mask.cat.raw" if i == MASK_DOWN else "mask.%s_%d.raw" % ("img" if m.group(1) == "img" else "lbl", i)
    m = re.match(r"flow_network_temp\.res_flow\.(\d+)\.", name)
    if m:
        return "mask.res_%s" % m.group(1)
    m = re.match(r"flow_network_temp\.up_flow\.(\d+)", name)
    if m:
        return "mask.up_%d.raw" % ((int(m.group(1)) - 1) // 2)
    return None


def first_tap(base, other, ignore=()):
    """The tap of the first tap-writing launch at or behind the first position where the two launch lists differ, on either
    side (None: the lists are equal).  Every launch in front of that position is the same launch on the same inputs."""
    a = [l for l in base if not l[0].endswith(tuple(ignore))] if ignore else list(base)
    b = [l for l in other if not l[0].endswith(tuple(ignore))] if ignore else list(other)
    i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), None)
    if i is None:
        return None if len(a) == len(b) else "<tail>"
    found = [next((t for t in (tap_of_launch(l[0]) for l in side[i:]) if t), None) for side in (a, b)]
    return found[0] if found[0] == found[1] else tuple(found)


def reordered_by_xcd(launches):
    """Launches whose grid xcd_chunk_of reorders: k_igemm and the head kernels with at least 64 tiles in a multiple of 8."""
    out = []
    for name, grid, tile in launches:
        tiles = int(grid.split(",")[0])
        if tile.startswith(("tile ", "head ")) and tiles >= 64 and tiles % 8 == 0:
            out.append(name)
    return out


# ---- GPU side -------------------------------------------------------------------------------------------------------------------
POISON, ZERO = 0xFF, 0x00
_shared = {}
_handles = {}


def shared(shape):
    """Checkpoint, inputs on the device and the oracle's frame of `shape`: computed once, never modified."""
    import torch                                          # noqa: F401
    from render_in_between_amd import synth
    if "spec" not in _shared:
        cfg = rib.hsm_gen_config()
        spec = rib.GenSpec.from_cfg(cfg)
        _shared.update(cfg=cfg, spec=spec, sd=synth.make_state_dict(spec, 0))
    if shape not in _shared:
        from oracle import generator_ref
        label, fake, prev = synth.make_inputs(_shared["spec"], *shape, INPUT_SEED)
        oimg, omask = generator_ref.RefGenerator(_shared["spec"], _shared["sd"])(label, None, fake, prev)
        _shared[shape] = dict(inputs=tuple(t.cuda() for t in (label, fake, prev)), oimg=oimg.cuda(), omask=omask.cuda())
    return _shared[shape]


def handle(monkeypatch, env, dtype="f32"):
    """A Generator of the full configuration built under `env`, which is set again on every call: plans are built lazily per
    shape, so the switch has to be in place whenever the handle is used.  One handle is kept at a time: asking for another
    drops the one before (what it rendered stays valid)."""
    clean_env(monkeypatch, env)
    key = (tuple(sorted(dict(env).items())), dtype)
    if key not in _handles:
        _handles.clear()
        shared(SHAPES[0])
        G = rib.Generator(_shared["cfg"], compute_dtype=dtype).eval()
        G.load_state_dict(_shared["sd"])
        _handles[key] = G
    return _handles[key]


Render = collections.namedtuple("Render", "img mask names taps launches")


def read_taps(G, shape):
    """([names], [device tensors]) of the last forward's taps, in plan order."""
    import torch
    B, H, W = shape
    ws = G._workspace(B, H, W)
    name = C.c_char_p(); ch = C.c_int(); th = C.c_int(); tw = C.c_int()
    names, out = [], []
    for i in range(G._lib.rib_num_taps(G._h, B, H, W)):
        _native.check(G._h, G._lib.rib_tap_info(G._h, B, H, W, i, C.byref(name), C.byref(ch), C.byref(th), C.byref(tw)))
        dst = torch.empty((B, ch.value, th.value, tw.value), dtype=torch.float32, device=G.device)
        _native.check(G._h, G._lib.rib_read_tap(G._h, B, H, W, i, C.c_void_p(ws.data_ptr()), C.c_void_p(dst.data_ptr()), G._stream()))
        names.append(name.value.decode()); out.append(dst)
    return names, out


def render(G, shape, taps, fill=POISON):
    """One frame of `shape` on a workspace whose every byte is `fill` (0xFF: NaN in fp32, bf16 and half, so that an element a
    launch reads without anybody having stored it shows; rib_forward clears nothing)."""
    import torch
    G.enable_taps(taps)                                   # rebuilds the plans when it changes; drops the cached workspaces
    B, H, W = shape
    label, fake, prev = shared(shape)["inputs"]
    launches = [(o["name"], o["grid"], o["tile"]) for o in G.launch_info(B, H, W)]
    G._workspace(B, H, W).fill_(fill)
    img, mask = G(label, None, fake, prev)
    names, tl = read_taps(G, shape) if taps else ([], [])
    torch.cuda.synchronize()
    return Render(img, mask, names, tl, launches)


def render_chain(G, shape, T=CHAIN_T, fill=POISON):
    """(imgs, masks, fuses) of one T-frame segment on workspaces (the frame's and the chain's) filled with `fill`."""
    import torch
    from render_in_between_amd import synth
    B, H, W = shape
    spec = _shared["spec"]
    frames = [synth.make_inputs(spec, B, H, W, INPUT_SEED + 1 + t) for t in range(T)]
    labels = torch.stack([f[0] for f in frames]).cuda()
    dains = torch.stack([f[1] for f in frames]).cuda()
    key = frames[0][2].cuda()
    G.enable_taps(False)
    G._workspace(B, H, W).fill_(fill)
    need = int(G._lib.rib_chain_workspace_bytes(G._h, T, B, H, W))
    G.__dict__.setdefault("_chain_ws", {})[(B, H, W)] = torch.full((max(need, 1),), fill, dtype=torch.uint8, device=G.device)
    out = G.chain(key, labels, dains)
    torch.cuda.synchronize()
    return out


def xcd_child(out_dir):
    """The switched side of the RIB_NO_XCD row: this process was started with the variable set and renders XCD_SHAPE once."""
    import pytest
    import torch
    assert os.environ.get("RIB_NO_XCD") == "1"
    mp = pytest.MonkeyPatch()
    try:
        G = handle(mp, {"RIB_NO_XCD": "1"})
        r = render(G, XCD_SHAPE, taps=False)
        torch.save({"img": r.img.cpu(), "mask": r.mask.cpu()}, os.path.join(out_dir, "xcd_off.pt"))
    finally:
        mp.undo()


if __name__ == "__main__":
    xcd_child(sys.argv[1])
