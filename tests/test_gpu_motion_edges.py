"""GPU half of the motion transformer's edge-shape suite: every kernel path of csrc/motion.hip that the table of
tests/motion_edges_common.py reaches, against the fp64 oracle (tests/test_motion_edges_cpu.py proves which paths those are).

ribm_forward is called through ctypes with buffers the test owns: `joints` and `reco` are slices of one allocation filled
with NaN, with 64 guard floats in front, between and behind; the workspace has every byte set to 0xFF before each run.  An
element that a launch fails to write therefore reads back as NaN, never as an earlier, correct value.

One test per case, so that a fault names its path:
  1. ribm_num_launches is what expected_launches restates from the dispatch
  2. NaN exactly where the fp64 oracle has NaN (A7: clip 1 and nothing of clip 0); the guards are untouched
  3. max |gpu - f64| over the non-NaN elements, for joints and reco separately, <= max(ERR_FACTOR * e32, ERR_FLOOR), where e32
     is the case's own fp32-oracle error against fp64 (2.5e-7 .. 7e-6 on this table).  A wrongly visible or wrongly hidden key
     moves the outputs by 5e-3 .. 2.6e-1, so the bound separates rounding from a wrong kernel by three orders of magnitude.
     ERR_FACTOR = 8 covers the kernels' sequential fmaf chains over K <= 1024 and L <= 1200, whose error can grow linearly
     where the oracle's blocked sums grow with about the square root, and the device's expf / erff against libm.  ERR_FLOOR is
     the figure tests/test_motion_gpu.py records as measured for this path (~1e-5); it matters only where e32 is tiny (L4).
     The suite's absolute 1e-4 stays asserted.  Every case writes both errors and their ratio to e32 to motion_edges.json in
     $RIB_REPORT_DIR (else test_reports/); profiles/r19_motion_edges.txt holds the figures of the first hardware run.
  4. for the cases marked `noise` (A3 in both dispatches, L1): noise in the padded and masked src frames leaves every frame
     that motion_edges_common.noise_plan calls valid bit-equal - in two modes, because with random masks the interpolation
     reads hidden key frames (see noise_plan)
  5. a second run of the same case is bit-equal (no atomics)
"""
import ctypes as C
import json
import os

import pytest
import torch

import render_in_between_amd  # noqa: F401
from render_in_between_amd.motion import model, synth, _native
from tests import motion_edges_common as mc

pytestmark = pytest.mark.gpu
REPORT_DIR = os.environ.get("RIB_REPORT_DIR") or "test_reports"
ERR_FACTOR = 8.0
ERR_FLOOR = 1e-5
ABS_BAR = 1e-4           # the bar of tests/test_motion_gpu.py
GUARD = 64
_report = {}


class Runner:
    """One handle with the case's weights, and ribm_forward on buffers poisoned before every run."""

    def __init__(self, spec):
        self.spec = spec
        self.T = model.MotionTransformer(spec, device="cuda:0").eval()
        self.T.load_state_dict(synth.make_state_dict(spec, mc.WEIGHT_SEED))
        self.lib, self.h, self.dev = self.T._lib, self.T._h, self.T.device

    def __call__(self, b, src, src_pos, tgt_pos):
        N, Cj, L = src.shape
        n_out = L * N * Cj
        dev = self.dev
        d_src = src.to(dev, torch.float32).contiguous(); d_tgt = b.tgt.to(dev, torch.float32).contiguous()
        d_sm = b.src_mask.to(dev, torch.uint8).contiguous(); d_tm = b.tgt_mask.to(dev, torch.uint8).contiguous()
        d_sp = src_pos.to(dev, torch.float32).contiguous(); d_tp = tgt_pos.to(dev, torch.float32).contiguous()
        out = torch.full((3 * GUARD + 2 * n_out,), float("nan"), dtype=torch.float32, device=dev)
        poison = out.view(torch.int32)[0].item()
        joints = out[GUARD:GUARD + n_out]
        reco = out[2 * GUARD + n_out:2 * GUARD + 2 * n_out]
        ws_bytes = int(self.lib.ribm_workspace_bytes(self.h, N, L))
        ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        _native.check(self.h, self.lib.ribm_forward(self.h, N, L, int(b.rate), p(d_src), p(d_sm), p(d_sp), p(d_tgt), p(d_tm), p(d_tp),
                                                    p(joints), p(reco), p(ws), ws_bytes, st))
        torch.cuda.synchronize()
        host = out.cpu()
        bits = host.view(torch.int32)
        for lo in (0, GUARD + n_out, 2 * GUARD + 2 * n_out):
            assert bool((bits[lo:lo + GUARD] == poison).all()), "guard floats at %d were written" % lo
        shape = (L, N, Cj)
        return host[GUARD:GUARD + n_out].view(shape).clone(), host[2 * GUARD + n_out:2 * GUARD + 2 * n_out].view(shape).clone()


def _write_report():
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "motion_edges.json"), "w") as f:
        json.dump(_report, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("cid", mc.CASE_IDS)
def test_motion_edge_case_against_fp64(cid, monkeypatch):
    case = mc.BY_ID[cid]
    spec = mc.spec_of(case)
    ref = mc.reference(cid)
    b = ref.batch
    if case.forced_stream:
        monkeypatch.setenv("RIBM_NO_TILE_ATTENTION", "1")
    else:
        monkeypatch.delenv("RIBM_NO_TILE_ATTENTION", raising=False)
    run = Runner(spec)
    joints, reco = run(b, b.src, ref.src_pos, ref.tgt_pos)
    # 1. the launch list
    assert run.lib.ribm_num_launches(run.h) == mc.expected_launches(spec)
    # 2. NaN where the oracle has NaN and nowhere else: nothing unwritten, nothing leaking out of a dead clip
    assert torch.equal(torch.isnan(joints), torch.isnan(ref.j64)), "joints: %d NaN, the oracle %d" % (int(torch.isnan(joints).sum()), int(torch.isnan(ref.j64).sum()))
    assert torch.equal(torch.isnan(reco), torch.isnan(ref.r64)), "reco: %d NaN, the oracle %d" % (int(torch.isnan(reco).sum()), int(torch.isnan(ref.r64).sum()))
    # 3. the error against fp64, in units of the fp32 oracle's own
    ej, er = mc.max_err(joints, ref.j64), mc.max_err(reco, ref.r64)
    bound = max(ERR_FACTOR * ref.e32, ERR_FLOOR)
    _report[cid] = {"e32": ref.e32, "err_joints": ej, "err_reco": er, "ratio_joints": ej / ref.e32, "ratio_reco": er / ref.e32,
                    "bound": bound, "N": len(case.lens), "L": max(case.lens), "features": sorted(mc.case_features(case))}
    _write_report()
    print("%s: gpu vs fp64 joints %.2e reco %.2e; fp32 oracle vs fp64 %.2e; ratios %.2f %.2f; bound %.2e"
          % (cid, ej, er, ref.e32, ej / ref.e32, er / ref.e32, bound))
    assert ej <= bound and er <= bound
    assert ej <= ABS_BAR and er <= ABS_BAR
    # 5. bit-reproducible
    j2, r2 = run(b, b.src, ref.src_pos, ref.tgt_pos)
    for x, y in ((joints, j2), (reco, r2)):
        assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(x[~torch.isnan(x)], y[~torch.isnan(y)])
    # 4. hidden frames are hidden
    if case.noise:
        checked = False
        for mode in ("all", "unread"):
            noisy, joints_ok, reco_ok = mc.noise_plan(spec, b, mode)
            assert bool(noisy.any())
            jn, rn = run(b, mc.with_noise(b, noisy, case.seed + 1), ref.src_pos, ref.tgt_pos)
            jo, ro = joints_ok.t(), reco_ok.t()
            assert bool(ro.any()) and torch.equal(rn[ro], reco[ro]), "%s: reco moved with noise in hidden frames (%s)" % (cid, mode)
            assert torch.equal(jn[jo], joints[jo]), "%s: joints moved with noise in hidden frames (%s)" % (cid, mode)
            checked = checked or bool(jo.any())
        assert checked and bool(mc.noise_plan(spec, b, "unread")[1].all())
