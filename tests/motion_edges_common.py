"""What tests/test_motion_edges_cpu.py and tests/test_gpu_motion_edges.py share: the table of edge-shape cases for stage 1
(csrc/motion.hip behind include/rib_motion.h), the batches they run on, their fp32 / fp64 oracle results, and a plain
restatement of the dispatch in `ribm_forward` - which kernel, instantiation and LDS class every attention takes, which
`linear()` calls split in two, which `km_linear` paths run, how many launches result.

The CPU file proves that the union of `features` over the table holds every path the table claims to reach (no GPU case is
vacuous) and pins the oracle figures the GPU bound is made of; the GPU file holds the kernels to the fp64 oracle.

Pure Python: importable without a GPU and without the shared library."""
import collections
import functools
import os
import re

import numpy as np
import torch

import render_in_between_amd  # noqa: F401
from render_in_between_amd.motion import MotionSpec, synth
from oracle import motion_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION_HIP = os.path.join(ROOT, "render-in-between_amd", "csrc", "motion.hip")
HEAD_DIMS = (8, 16, 32, 64)
WEIGHT_SEED = 11
NOISE_SIGMA = 10.0

# km_linear's tiling (csrc/motion.hip: TM rows x TN columns per block, W^T in KC-row chunks, inputs staged 2048 at a time)
TM, TN, KC, STAGE = 8, 64, 128, 2048
SMALL_K = 256                     # K <= 256: LayerNorm / positional prologue path, one staging batch
INTERP_GRID_MAX = 1024            # km_interp: at most 1024 blocks of 256 threads, grid-stride beyond
DEFAULT_DYNAMIC_LDS = 64 * 1024   # what a launch may ask for without hipFuncSetAttribute


# ---------------------------------------------------------------- the tile / streamed switch, read out of the source
def attn_tile_lds_bytes(hd, L):
    """attn_tile_lds_bytes<HD>(Lk) of csrc/motion.hip: S[QT][L + 1], V[L][HD], q[QT][HD], sum[QT], floats."""
    qt = 256 // hd
    return (qt * (L + 1) + L * hd + qt * hd + qt) * 4


def _const_expr(text):
    if not re.fullmatch(r"[0-9 *+()]+", text):
        raise AssertionError("not a constant product: %r" % text)
    return int(eval(text, {"__builtins__": {}}))


@functools.lru_cache(maxsize=None)
def tile_lds_limits():
    """{head_dim: bytes}: the dispatch bound (`lds <= ATTN_TILE_LDS_MAX`) capped by what ribm_create allows each
    km_attention_tile<HD> through hipFuncSetAttribute.  Fails if either text is no longer found."""
    with open(MOTION_HIP) as f:
        src = f.read()
    m = re.search(r"constexpr\s+size_t\s+ATTN_TILE_LDS_MAX\s*=\s*([^;]+);", src)
    assert m, "ATTN_TILE_LDS_MAX not found in csrc/motion.hip"
    dispatch = _const_expr(m.group(1).strip())
    assert re.search(r"lds\s*<=\s*ATTN_TILE_LDS_MAX", src), "the tile / streamed switch no longer reads `lds <= ATTN_TILE_LDS_MAX`"
    per = dict(re.findall(r"&km_attention_tile<(\d+)>\)\s*,\s*hipFuncAttributeMaxDynamicSharedMemorySize\s*,\s*\(int\)\s*([^)]+)\)", src))
    assert sorted(int(k) for k in per) == list(HEAD_DIMS), "per-handle dynamic LDS limits not found for every head_dim: %s" % sorted(per)
    out = {}
    for hd in HEAD_DIMS:
        v = per[str(hd)].strip()
        out[hd] = min(dispatch, dispatch if v == "ATTN_TILE_LDS_MAX" else _const_expr(v))
    return out


def tile_lmax(hd):
    """The largest L whose score tile still takes km_attention_tile<hd>."""
    lim = tile_lds_limits()[hd]
    L = 2
    while attn_tile_lds_bytes(hd, L + 1) <= lim:
        L += 1
    assert attn_tile_lds_bytes(hd, L) <= lim < attn_tile_lds_bytes(hd, L + 1)
    return L


# ---------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "id over lens rate mask seed forced_stream dead noise why")


def _hd_over(hd):
    return {8: dict(hidden_dim=16, pos_hidden_dim=16, nheads=2), 16: dict(), 32: dict(hidden_dim=32, pos_hidden_dim=32, nheads=1),
            64: dict(hidden_dim=64, pos_hidden_dim=64, nheads=1)}[hd]


def _spec_over(D, H, F, C, **kw):
    return dict(hidden_dim=D, pos_hidden_dim=D, nheads=H, dim_feedforward=F, input_joints=C, **kw)


def _cases():
    one = dict(enc_layers=1, dec_layers=1)
    out = []

    def add(id, over, lens, rate, mask="keys", forced_stream=False, dead=(), noise=False, why=""):
        o = dict(one); o.update(over)
        out.append(Case(id, o, tuple(lens), rate, mask, 100 + 7 * len(out), forced_stream, tuple(dead), noise, why))
    # linear paths (small L, tiled attention)
    add("L1", _spec_over(24, 3, 300, 1), [19, 13], 2, noise=True,
        why="QKV and KV split; wide K = 300 (44-wide last chunk, second 2048-batch partial); K = 1; Nout = 1; R % 8 = 6")
    add("L2", _spec_over(40, 5, 1000, 70), [21], 4, why="split with an 80-column first launch; K = 1000; C in two column blocks, the second partial")
    add("L3", _spec_over(48, 3, 257, 128), [9, 9, 5], 2, why="K = 257 (chunks 128, 128, 1); C = 128")
    add("L4", _spec_over(8, 1, 1, 2, pre_norm=False, activation="relu"), [3], 2, why="the smallest accepted model; km_layernorm at D < 64")
    add("L5", _spec_over(256, 4, 256, 38, activation="gelu", two_stage=False), [17], 16, why="K = 256, the last small-path K; head_dim 64")
    add("L6", _spec_over(248, 31, 255, 38, pre_norm=False), [11, 7], 2, why="LayerNorm prologue and km_layernorm at K = 3 * 64 + 56; 31 heads")
    # attention paths
    add("A1", {}, [601], 8, why="tiled attention with 77 KB of LDS, as the folder driver calls it for a 600-frame clip")
    for hd in HEAD_DIMS:
        add("A2-hd%d-tile" % hd, _hd_over(hd), [tile_lmax(hd)], 1, "random", why="the largest L on the tiled side of the switch")
        add("A2-hd%d-stream" % hd, _hd_over(hd), [tile_lmax(hd) + 1], 1, "random", why="the smallest L on the streamed side of the switch")
    for hd in HEAD_DIMS:
        for forced in (False, True):
            add("A3-hd%d-%s" % (hd, "stream" if forced else "tile"), _hd_over(hd), [131, 65, 67], 2, "random", forced_stream=forced, noise=True,
                why="three key tiles (the last of 3 keys), three query blocks, ragged masks")
    for hd in (8, 32, 64):
        add("A4-hd%d" % hd, _hd_over(hd), [259, 257], 2, "random", why="the tile kernel's second key sweep (3 threads)")
    add("A5", dict(enc_layers=6, dec_layers=6), [131, 129, 3], 2, why="depth: the default spec's 6 + 6 layers on a ragged batch")
    add("A6", dict(input_joints=128), [689, 689, 689], 8, why="km_interp grid-stride (264 576 elements)")
    add("A7", {}, [33, 33], 8, dead=(1,), why="a clip whose keys are all masked: NaN stays inside its clip")
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}


def spec_of(case):
    return MotionSpec(**case.over)


# ---------------------------------------------------------------- batches
Batch = collections.namedtuple("Batch", "src tgt src_mask tgt_mask lens rate")


def batch(spec, lens, rate, seed, mask="keys", dead=()):
    """N clips of the given lengths (synth.make_clip), zero-padded at the end to max(lens); both masks True on the padding.
    "keys": the masks of make_clip (every non-key frame hidden from the encoder, nothing from the decoder).  "random": the src
    mask is seeded noise, about half masked, frames 0 and l - 1 visible; about a tenth of the tgt mask is set.  `dead`: clips
    whose src mask is True everywhere."""
    assert mask in ("keys", "random")
    N, L, C = len(lens), max(lens), spec.input_joints
    src = torch.zeros(N, C, L); tgt = torch.zeros(N, C, L)
    sm = torch.ones(N, L, dtype=torch.bool); tm = torch.ones(N, L, dtype=torch.bool)
    for n, l in enumerate(lens):
        assert l >= 2 and (l - 1) % rate == 0, "clip length %d is not n_key frames at rate %d" % (l, rate)
        inp, interp, em, dm = synth.make_clip(spec, (l - 1) // rate + 1, rate, seed + n)
        if mask == "random":
            rng = np.random.default_rng([int(seed), n, 7003])
            e = rng.random(l) < 0.5
            e[0] = e[l - 1] = False
            d = rng.random(l) < 0.1
            d[int(rng.integers(l))] = False                  # never a clip without a visible decoder key
            em, dm = torch.from_numpy(e), torch.from_numpy(d)
            inp = interp * (~em).view(1, -1)
        src[n, :, :l] = inp; tgt[n, :, :l] = interp
        sm[n, :l] = em; tm[n, :l] = dm
    for n in dead:
        sm[n] = True
    return Batch(src, tgt, sm, tm, tuple(lens), rate)


def case_batch(case):
    return batch(spec_of(case), case.lens, case.rate, case.seed, case.mask, case.dead)


def positions(spec, b):
    npf = spec.pos_hidden_dim // 2
    return motion_ref.position_embedding_sine(b.src_mask, npf), motion_ref.position_embedding_sine(b.tgt_mask, npf)


Reference = collections.namedtuple("Reference", "batch src_pos tgt_pos j32 r32 j64 r64 e32")


def max_err(a, b):
    """max |a - b| over the elements where neither is NaN (0 if there is none)."""
    a, b = a.double(), b.double()
    ok = ~(torch.isnan(a) | torch.isnan(b))
    return float((a - b)[ok].abs().max()) if bool(ok.any()) else 0.0


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The case's batch with its fp32 and fp64 oracle outputs, computed once per process and shared by every test that needs
    them (treat as read-only).  e32 = max |f32 - f64| over the non-NaN elements of joints and reco."""
    case = BY_ID[case_id]
    spec = spec_of(case)
    sd = synth.make_state_dict(spec, WEIGHT_SEED)
    b = case_batch(case)
    sp, tp = positions(spec, b)
    cfg = spec.as_dict()
    with torch.no_grad():
        j32, r32 = motion_ref.transformer_forward(sd, cfg, b.src, b.src_mask, sp, b.tgt, b.tgt_mask, tp, b.rate)
        j64, r64 = motion_ref.transformer_forward_f64(sd, cfg, b.src, b.src_mask, sp, b.tgt, b.tgt_mask, tp, b.rate)
    return Reference(b, sp, tp, j32, r32, j64, r64, max(max_err(j32, j64), max_err(r32, r64)))


# ---------------------------------------------------------------- noise in the frames nobody may look at
def noise_plan(spec, b, mode):
    """Which src frames get noise, and on which frames the outputs must then be bit-equal: -> (noisy, joints_ok, reco_ok),
    bool [N][L] each.

    mode "all": every padded or masked frame of src.  Attention hides those frames as keys, so reco - the encoder's output
    plus its input, frame by frame - keeps every visible frame.  With two_stage the decoder's input is interpolated from
    reco at the multiples of `rate` (and the last frame) whether or not those were visible, so a frame of `center` that reads
    a noisy frame is dirty; the decoder hides it only if the tgt mask does.  If every dirty frame is hidden, joints keeps
    every clean frame; if one is visible as a decoder key, every joint may move and joints_ok is empty.
    mode "unread": the padded and masked frames that the interpolation does not read.  Then `center` is clean, what is
    left to hide the noise is the encoder's and the cross attention's key masks, and joints keeps every frame."""
    assert mode in ("all", "unread")
    sm, tm = b.src_mask, b.tgt_mask
    N, L = sm.shape
    noisy = sm.clone()
    idx = torch.arange(L)
    if spec.two_stage:
        prev = idx // b.rate * b.rate
        nxt = torch.clamp((idx // b.rate + 1) * b.rate, max=L - 1)
        rem = idx % b.rate
        if mode == "unread":
            read = torch.zeros(L, dtype=torch.bool)
            read[prev] = True; read[nxt[rem > 0]] = True; read[L - 1] = True
            noisy = noisy & ~read.view(1, L)
        dirty = noisy[:, prev] | (noisy[:, nxt] & (rem > 0).view(1, L))
    else:
        dirty = torch.zeros_like(sm)
    joints_ok = torch.zeros_like(sm) if bool((dirty & ~tm).any()) else ~dirty
    return noisy, joints_ok, ~sm


def with_noise(b, noisy, seed):
    """src with seeded N(0, NOISE_SIGMA^2) noise in the frames `noisy` marks."""
    g = torch.Generator().manual_seed(int(seed))
    n = torch.randn(b.src.shape, generator=g) * NOISE_SIGMA
    return torch.where(noisy.unsqueeze(1), n, b.src)


# ---------------------------------------------------------------- the dispatch of ribm_forward, restated
def _linear_launches(has_pos, pos_cols, nout):
    """linear(): a TN-column block must not straddle the pos / no-pos boundary, else two launches."""
    return 2 if has_pos and pos_cols < nout and pos_cols % TN != 0 else 1


def expected_launches(spec):
    """What ribm_num_launches reports after a forward of this spec (kernel launches; the device-to-device copies do not count)."""
    D = spec.hidden_dim
    ln = 0 if spec.pre_norm else 1
    ffn = 2
    qkv = _linear_launches(True, 2 * D, 3 * D)
    q = _linear_launches(True, D, D)
    kv = _linear_launches(True, D, 2 * D)
    n = 1                                                        # input_embed(src)
    n += spec.enc_layers * (qkv + 1 + 1 + ln + ffn + ln)         # in_proj, attention, out_proj, [norm1], FFN, [norm2]
    n += 1 if spec.pre_norm else 0                               # encoder.norm
    n += 1                                                       # joints_embed -> reco
    n += 1 if spec.two_stage else 0                              # km_interp
    n += 1                                                       # input_embed(center)
    n += spec.dec_layers * (qkv + 1 + 1 + ln + q + kv + 1 + 1 + ln + ffn + ln)
    n += 1                                                       # decoder.norm + joints_embed
    return n


def features(spec, N, L, forced_stream=False, lens=None, src_mask=None, tgt_mask=None):
    """The set of code paths of csrc/motion.hip that one forward of `spec` on N clips of L frames takes.  lens and the masks
    (bool [N][L]) add the properties of the batch itself."""
    f = set()
    D, F, C, H = spec.hidden_dim, spec.dim_feedforward, spec.input_joints, spec.nheads
    hd = D // H
    R = N * L
    # attention()
    lds = attn_tile_lds_bytes(hd, L)
    if lds <= tile_lds_limits()[hd] and not forced_stream:
        f.add("km_attention_tile<%d>" % hd)
        f.add("km_attention_tile<%d>:lds%s64K" % (hd, ">" if lds > DEFAULT_DYNAMIC_LDS else "<="))
        if L > 256:
            f.add("km_attention_tile<%d>:second_key_sweep" % hd)
        if L == tile_lmax(hd):
            f.add("switch<%d>:largest_tiled_L" % hd)
    else:
        f.add("km_attention<%d>" % hd)
        if not forced_stream and L == tile_lmax(hd) + 1:
            f.add("switch<%d>:smallest_streamed_L" % hd)
        if L > 64 and L % 64:
            f.add("km_attention:partial_last_key_tile")
            for m in (src_mask, tgt_mask):
                if m is not None and bool(m[:, L // 64 * 64:].any()):
                    f.add("km_attention:masked_key_in_partial_last_key_tile")
        if L > 64:
            f.add("km_attention:several_query_blocks")
    # linear()
    if _linear_launches(True, 2 * D, 3 * D) == 2:
        f.add("linear:qkv_split")
        if 2 * D > TN:
            f.add("linear:qkv_split:first_launch_of_two_column_blocks")
    if _linear_launches(True, D, 2 * D) == 2:
        f.add("linear:kv_split")
        if D != 32:
            f.add("linear:kv_split:D!=32")
    for K in (C, D, F):                                           # input_embed; every projection; linear2
        if K > SMALL_K:
            f.add("km_linear:wide")
            if K % KC:
                f.add("km_linear:wide:K%128!=0")
            if (TM * K) % STAGE:
                f.add("km_linear:wide:8K%2048!=0")
        for k in (1, 256, 257):
            if K == k:
                f.add("km_linear:K==%d" % k)
    if D % 64:                                                    # decoder.norm is a prologue in every spec
        f.add("km_linear:ln_prologue:K%64!=0")
        f.add("km_layernorm:D%64!=0")                             # encoder.norm (pre-norm) or the layers' own (post-norm)
    if D < 64:
        f.add("km_layernorm:D<64")
    if not spec.pre_norm:
        f.add("post_norm")
    if R % TM:
        f.add("km_linear:partial_row_block")
    if C == 1:
        f.add("input_joints==1")
        f.add("km_linear:Nout==1")
    if TN < C < 2 * TN:
        f.add("input_joints:two_column_blocks_second_partial")
    if C == 2 * TN:
        f.add("input_joints==128")
    # km_interp
    if spec.two_stage:
        f.add("km_interp")
        if R * C > INTERP_GRID_MAX * 256:
            f.add("km_interp:grid_stride")
    # the batch
    if lens is not None and len(set(lens)) > 1:
        f.add("batch:clips_of_different_lengths")
    if src_mask is not None and N > 1 and bool(src_mask.all(dim=1).any()) and not bool(src_mask.all()):
        f.add("batch:one_clip_entirely_masked")
    return f


def case_features(case):
    b = case_batch(case)
    return features(spec_of(case), len(case.lens), max(case.lens), case.forced_stream, case.lens, b.src_mask, b.tgt_mask)
