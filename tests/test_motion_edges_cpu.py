"""CPU half of the motion transformer's edge-shape suite (tests/motion_edges_common.py holds the table).

  * every case is a configuration the product accepts (MotionSpec.validate, a host-only ribm_create)
  * the coverage claim is itself tested: the union of `features` over the table holds every path listed in REQUIRED, the
    paths of csrc/motion.hip that tests/test_motion_gpu.py never takes
  * the fp32 oracle against the fp64 oracle on every case: the error the GPU bound is a multiple of, held to the bar the CPU
    suite already holds the oracle to (2e-5); the figures go to motion_edges_cpu.json in $RIB_REPORT_DIR (else test_reports/)
  * in fp64, noise in the src frames that no attention may look at leaves every frame that noise_plan calls valid bit-equal:
    the property the GPU file then asks of the kernels
"""
import ctypes as C
import json
import os

import pytest
import torch

import render_in_between_amd  # noqa: F401
from render_in_between_amd.motion import synth, _native
from oracle import motion_ref
from tests import motion_edges_common as mc

REPORT_DIR = os.environ.get("RIB_REPORT_DIR") or "test_reports"
E32_BAR = 2e-5
_report = {}

HD = mc.HEAD_DIMS
REQUIRED = (
    # the streamed kernel in every instantiation, and both sides of the switch for every head_dim
    ["km_attention<%d>" % hd for hd in HD]
    + ["switch<%d>:largest_tiled_L" % hd for hd in HD] + ["switch<%d>:smallest_streamed_L" % hd for hd in HD]
    # the tile kernel above the default 64 KB of dynamic LDS, and its second key sweep where no earlier test has one
    + ["km_attention_tile<%d>:lds>64K" % hd for hd in HD]
    + ["km_attention_tile<%d>:second_key_sweep" % hd for hd in (8, 32, 64)]
    # linear(): both splits; km_linear: the wide path off its round sizes, the sizes around the small / wide threshold,
    # the LayerNorm prologue with a partial last 64
    + ["linear:qkv_split", "linear:qkv_split:first_launch_of_two_column_blocks", "linear:kv_split:D!=32",
       "km_linear:wide:K%128!=0", "km_linear:wide:8K%2048!=0", "km_linear:K==256", "km_linear:K==257", "km_linear:K==1",
       "km_linear:ln_prologue:K%64!=0", "km_layernorm:D%64!=0", "km_layernorm:D<64", "km_linear:Nout==1",
       "km_linear:partial_row_block"]
    # input_joints other than 38 and 6
    + ["input_joints==1", "input_joints:two_column_blocks_second_partial", "input_joints==128"]
    + ["km_interp:grid_stride"]
    # ragged batches
    + ["batch:clips_of_different_lengths", "km_attention:masked_key_in_partial_last_key_tile", "batch:one_clip_entirely_masked"]
)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        from importlib import util
        spec = util.spec_from_file_location("rib_build", os.path.join(os.path.dirname(_native.LIB_PATH), "build.py"))
        mod = util.module_from_spec(spec); spec.loader.exec_module(mod)
        mod.build()
    return _native.lib()


def test_switch_lengths_are_computed_from_the_source():
    assert {hd: mc.tile_lmax(hd) for hd in HD} == {8: 952, 16: 1191, 32: 953, 64: 560}     # with today's constants
    for hd in HD:
        lim = mc.tile_lds_limits()[hd]
        assert mc.attn_tile_lds_bytes(hd, mc.tile_lmax(hd)) <= lim < mc.attn_tile_lds_bytes(hd, mc.tile_lmax(hd) + 1)
    # where the > 64 KB class starts
    first = {hd: next(L for L in range(2, 2000) if mc.attn_tile_lds_bytes(hd, L) > mc.DEFAULT_DYNAMIC_LDS) for hd in HD}
    assert first == {8: 402, 16: 504, 32: 403, 64: 238}


@pytest.mark.parametrize("cid", mc.CASE_IDS)
def test_case_is_accepted_by_spec_and_native_create(lib, cid):
    case = mc.BY_ID[cid]
    s = mc.spec_of(case)
    s.validate()
    cfg = _native.RibmConfig(input_joints=s.input_joints, hidden_dim=s.hidden_dim, nheads=s.nheads, dim_feedforward=s.dim_feedforward,
                             enc_layers=s.enc_layers, dec_layers=s.dec_layers, activation=_native.ACT_IDS[s.activation],
                             pre_norm=int(s.pre_norm), two_stage=int(s.two_stage))
    h = C.c_void_p()
    assert lib.ribm_create(C.byref(cfg), -1, C.byref(h)) == 0, lib.ribm_last_error(None)
    assert lib.ribm_workspace_bytes(h, len(case.lens), max(case.lens)) > 0
    lib.ribm_destroy(h)
    for l in case.lens:
        assert l >= 2 and (l - 1) % case.rate == 0
    b = mc.case_batch(case)
    for n, l in enumerate(case.lens):                                   # both masks cover the padding
        assert bool(b.src_mask[n, l:].all()) and bool(b.tgt_mask[n, l:].all()) and not bool(b.src[n, :, l:].any())
        if n not in case.dead:
            assert not bool(b.src_mask[n, 0]) and not bool(b.src_mask[n, l - 1]) and not bool(b.tgt_mask[n, :l].all())
    if case.mask == "random":
        n_in = sum(case.lens)
        assert 0.3 * n_in <= int(b.src_mask.sum()) - (b.src_mask.numel() - n_in) <= 0.7 * n_in or n_in < 40


def test_case_table_reaches_every_path_it_claims():
    reached = {}
    for case in mc.CASES:
        for f in mc.case_features(case):
            reached.setdefault(f, []).append(case.id)
    missing = [f for f in REQUIRED if f not in reached]
    assert not missing, "no case reaches %s" % missing
    # what the rows of the table say of themselves
    want = {"L1": ["linear:qkv_split", "linear:kv_split", "km_linear:wide:K%128!=0", "km_linear:wide:8K%2048!=0", "km_linear:K==1",
                   "km_linear:Nout==1", "km_linear:partial_row_block", "batch:clips_of_different_lengths"],
            "L2": ["linear:qkv_split:first_launch_of_two_column_blocks", "km_linear:wide:K%128!=0", "input_joints:two_column_blocks_second_partial"],
            "L3": ["km_linear:K==257", "input_joints==128"],
            "L4": ["km_layernorm:D<64", "post_norm", "km_linear:K==1"],
            "L5": ["km_linear:K==256", "km_attention_tile<64>"],
            "L6": ["km_linear:ln_prologue:K%64!=0", "km_layernorm:D%64!=0", "post_norm"],
            "A1": ["km_attention_tile<16>:lds>64K", "km_attention_tile<16>:second_key_sweep"],
            "A5": ["batch:clips_of_different_lengths"],
            "A6": ["km_interp:grid_stride", "input_joints==128"],
            "A7": ["batch:one_clip_entirely_masked"]}
    for hd in HD:
        want["A2-hd%d-tile" % hd] = ["switch<%d>:largest_tiled_L" % hd, "km_attention_tile<%d>:lds>64K" % hd]
        want["A2-hd%d-stream" % hd] = ["switch<%d>:smallest_streamed_L" % hd, "km_attention<%d>" % hd]
        want["A3-hd%d-tile" % hd] = ["km_attention_tile<%d>:lds<=64K" % hd, "batch:clips_of_different_lengths"]
        want["A3-hd%d-stream" % hd] = ["km_attention<%d>" % hd, "km_attention:masked_key_in_partial_last_key_tile",
                                       "km_attention:several_query_blocks"]
    for hd in (8, 32, 64):
        want["A4-hd%d" % hd] = ["km_attention_tile<%d>:second_key_sweep" % hd]
    assert sorted(want) == sorted(mc.CASE_IDS)
    for cid, fs in want.items():
        got = mc.case_features(mc.BY_ID[cid])
        assert not [f for f in fs if f not in got], (cid, [f for f in fs if f not in got])
    # the two cases of a switch differ in nothing but one frame
    for hd in HD:
        a, b = mc.BY_ID["A2-hd%d-tile" % hd], mc.BY_ID["A2-hd%d-stream" % hd]
        assert a.over == b.over and b.lens[0] == a.lens[0] + 1


def test_expected_launches_of_known_specs():
    from render_in_between_amd.motion import MotionSpec
    # no split at D = 128; 90 is also what profiles/r06_motion_bench.json records from the hardware
    assert mc.expected_launches(MotionSpec()) == 1 + 6 * 5 + 1 + 1 + 1 + 1 + 6 * 9 + 1 == 90
    s = MotionSpec(hidden_dim=32, pos_hidden_dim=32, nheads=1, enc_layers=1, dec_layers=1)          # D = 32: the KV split only
    assert mc.expected_launches(s) == mc.expected_launches(MotionSpec(enc_layers=1, dec_layers=1)) + 1
    l1 = mc.spec_of(mc.BY_ID["L1"])                                                                # D = 24: QKV twice and KV
    assert mc.expected_launches(l1) == mc.expected_launches(MotionSpec(enc_layers=1, dec_layers=1)) + 3
    l4 = mc.spec_of(mc.BY_ID["L4"])                                                                # post-norm: 2 + 3 km_layernorm, no encoder.norm
    assert mc.expected_launches(l4) == mc.expected_launches(MotionSpec(enc_layers=1, dec_layers=1)) + 3 - 1 + 5


@pytest.mark.parametrize("cid", mc.CASE_IDS)
def test_fp32_oracle_against_fp64_oracle(cid):
    case = mc.BY_ID[cid]
    ref = mc.reference(cid)
    assert ref.j64.dtype == torch.float64 and ref.r64.dtype == torch.float64 and ref.j32.dtype == torch.float32
    assert torch.equal(torch.isnan(ref.j32), torch.isnan(ref.j64)) and torch.equal(torch.isnan(ref.r32), torch.isnan(ref.r64))
    nan_clip = torch.isnan(ref.j64).all(dim=2).all(dim=0)                      # [N]
    assert nan_clip.tolist() == [n in case.dead for n in range(len(case.lens))]
    assert bool(torch.isnan(ref.j64).any(dim=2).any(dim=0).equal(nan_clip)) and torch.equal(torch.isnan(ref.r64).all(dim=2).all(dim=0), nan_clip)
    _report[cid] = {"e32": ref.e32, "e32_joints": mc.max_err(ref.j32, ref.j64), "e32_reco": mc.max_err(ref.r32, ref.r64),
                    "max_abs_joints": float(torch.nan_to_num(ref.j64).abs().max()), "N": len(case.lens), "L": max(case.lens)}
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "motion_edges_cpu.json"), "w") as f:
        json.dump(_report, f, indent=1, sort_keys=True)
    print("%s: fp32 oracle vs fp64 oracle %.2e" % (cid, ref.e32))
    assert ref.e32 <= E32_BAR


@pytest.mark.parametrize("cid", mc.CASE_IDS)
def test_fp64_oracle_ignores_noise_in_hidden_frames(cid):
    case = mc.BY_ID[cid]
    spec = mc.spec_of(case)
    ref = mc.reference(cid)
    b = ref.batch
    sd = synth.make_state_dict(spec, mc.WEIGHT_SEED)
    checked_joints = False
    for mode in ("all", "unread"):
        noisy, joints_ok, reco_ok = mc.noise_plan(spec, b, mode)
        if not bool(noisy.any()):                  # rate 1: the interpolation reads every frame
            continue
        src = mc.with_noise(b, noisy, case.seed + 1)
        assert torch.equal(src[~noisy.unsqueeze(1).expand_as(src)], b.src[~noisy.unsqueeze(1).expand_as(src)])
        with torch.no_grad():
            j, r = motion_ref.transformer_forward_f64(sd, spec.as_dict(), src, b.src_mask, ref.src_pos, b.tgt, b.tgt_mask, ref.tgt_pos, b.rate)
        live = ~torch.isnan(ref.j64).any(dim=2).t()                           # [N][L]: A7's dead clip is NaN on both sides
        jo, ro = (joints_ok & live).t(), (reco_ok & live).t()                 # [L][N]
        assert torch.equal(j[jo], ref.j64[jo]) and torch.equal(r[ro], ref.r64[ro]), (cid, mode)
        assert not torch.isnan(j[jo]).any() and not torch.isnan(r[ro]).any()
        checked_joints = checked_joints or bool(jo.any())
        if mode == "unread":
            assert bool(joints_ok.all())
    assert checked_joints or not case.noise, "%s: no mode leaves a joint to compare" % cid
    if case.noise and case.mask == "random":
        # the random masks hide key frames the interpolation reads: with noise in ALL hidden frames the joints do move,
        # which is why the GPU test needs the second mode
        assert not bool(mc.noise_plan(spec, b, "all")[1].any())
