"""The interpolated background at the key frames' own size on the MI355X: rib_scaled_frames (csrc/mci.hip.h,
Generator.mci_frames_scaled) against the integer definition background.mci_frames_scaled_host, bit for bit."""
import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, synth

pytestmark = pytest.mark.gpu

_G = {}


def handle():
    if "g" not in _G:
        cfg = rib.hsm_gen_config()
        G = rib.Generator(cfg, device="cuda:0").eval()
        G.load_state_dict(synth.make_state_dict(rib.GenSpec.from_cfg(cfg), 0))
        _G["g"] = G
    return _G["g"]


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def random_field(B, H, W, amp, seed):
    """int16 [B, Hb, Wb, 2] in -amp..amp with both extreme components present in every segment."""
    Hb, Wb = bg.field_shape(H, W)
    f = np.random.default_rng(seed).integers(-amp, amp + 1, (B, Hb, Wb, 2)).astype(np.int16)
    f[:, 0, 0], f[:, -1, -1] = (amp, -amp), (-amp, amp)
    return f


def host(a0, b0, f, model, s, ks, border, precision):
    """The definition of a batch: uint8 [len(ks), B, h0, w0, 3]."""
    return np.stack([bg.mci_frames_scaled_host(a0[i], b0[i], f[i], model, s, ks, border=border, precision=precision) for i in range(len(a0))], 1)


def dev(G, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(G.device) for x in arrays)


VARIANTS = [("clamp", "full", 79), ("valid", "full", 79), ("clamp", "half", 159), ("valid", "half", 159)]
# (H, W) -> (h0, w0): enlargement beyond one workgroup pass (240 > 4 * 32), reduction, the odd width (byte stores), a tiny frame,
# the smallest frame at the largest ratio, equal sizes
PAIRS = [((64, 64), (136, 240)), ((64, 64), (48, 100)), ((32, 32), (31, 33)), ((64, 96), (7, 9)), ((16, 16), (1, 1)), ((64, 64), (64, 64))]


@pytest.mark.parametrize("model,size", PAIRS)
def test_size_pairs_equal_the_definition(model, size):
    G = handle()
    B, s, k_first, T = 2, 8, 3, 3
    a0, b0 = noise((B,) + size + (3,), 1), noise((B,) + size + (3,), 2)
    for border, precision, amp in VARIANTS:
        f = random_field(B, *model, amp, 3)
        want = host(a0, b0, f, model, s, range(k_first, k_first + T), border, precision)
        ta, tb, tf = dev(G, a0, b0, f)
        got = G.mci_frames_scaled(ta, tb, tf, model, s, k_first=k_first, count=T, border=border, precision=precision)
        assert got.shape == (T, B) + size + (3,) and got.dtype == torch.uint8
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (border, precision)
        if model == size:                                            # ... and rib_mci_frames' own uint8 output
            same = G.mci_frames(ta, tb, tf, s, k_first=k_first, count=T, normalised=False, border=border, precision=precision)
            assert torch.equal(got, same)


def test_the_key_frames_and_the_default_range():
    G = handle()
    model, size, s = (32, 32), (31, 33), 4
    a0, b0, f = noise((1,) + size + (3,), 4), noise((1,) + size + (3,), 5), random_field(1, *model, 79, 6)
    ta, tb, tf = dev(G, a0, b0, f)
    out = G.mci_frames_scaled(ta[0], tb[0], tf[0], model, s, border="valid")          # [h0,w0,3] key frames: frames 0 .. s-1
    assert out.shape == (s,) + size + (3,)
    assert torch.equal(out[0], ta[0])
    assert torch.equal(out.cpu(), torch.from_numpy(host(a0, b0, f, model, s, range(s), "valid", "full")[:, 0]))
    last = G.mci_frames_scaled(ta, tb, tf, model, s, k_first=s, count=1)
    assert torch.equal(last[0], tb)


def test_the_int32_bound():
    """Every component +-159 in half pixels, ratio 16, s = 1024: unit * k * DS reaches 666 894 336."""
    G = handle()
    model, size, s = (8, 8), (128, 128), 1024
    a0, b0 = noise((2,) + size + (3,), 7), noise((2,) + size + (3,), 8)
    f = np.empty((2, 1, 1, 2), np.int16)
    f[0, 0, 0], f[1, 0, 0] = (159, -159), (-159, 159)
    ta, tb, tf = dev(G, a0, b0, f)
    for border in bg.BORDERS:
        for k_first in (1021, 1):
            want = host(a0, b0, f, model, s, range(k_first, k_first + 3), border, "half")
            got = G.mci_frames_scaled(ta, tb, tf, model, s, k_first=k_first, count=3, border=border, precision="half")
            assert torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("border,precision", [("clamp", "full"), ("valid", "half")])
def test_a_searched_field(border, precision):
    """The field of G.mci_field (and G.mci_refine) itself, from resized key frames of a moving scene."""
    from render_in_between_amd import resize
    G = handle()
    model, size, s = (64, 80), (160, 200), 4
    big = noise((size[0] // 8 + 3, size[1] // 8 + 3, 3), 9)
    big = np.repeat(np.repeat(big, 8, 0), 8, 1)
    a0, b0 = big[8:8 + size[0], 8:8 + size[1]], big[4:4 + size[0], 14:14 + size[1]]
    a, b = resize.resize_cubic_u8(a0, model[1], model[0]), resize.resize_cubic_u8(b0, model[1], model[0])
    ta, tb, ta0, tb0 = dev(G, a, b, a0, b0)
    field = G.mci_field(ta, tb, border=border)
    if precision == "half":
        field = G.mci_refine(ta, tb, field, border=border)
    assert field.any()
    got = G.mci_frames_scaled(ta0, tb0, field, model, s, k_first=1, border=border, precision=precision)
    want = bg.mci_frames_scaled_host(np.ascontiguousarray(a0), np.ascontiguousarray(b0), field.cpu().numpy(), model, s, range(1, s), border=border, precision=precision)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_a_frame_does_not_depend_on_T_or_B():
    G = handle()
    model, size, s = (64, 64), (48, 100), 8
    a0, b0, f = noise((3,) + size + (3,), 10), noise((3,) + size + (3,), 11), random_field(3, *model, 79, 12)
    ta, tb, tf = dev(G, a0, b0, f)
    three = G.mci_frames_scaled(ta, tb, tf, model, s, k_first=4, count=3, border="valid")
    for b_ in range(3):
        alone = G.mci_frames_scaled(ta[b_], tb[b_], tf[b_], model, s, k_first=5, count=1, border="valid")
        assert torch.equal(alone[0], three[1, b_])                   # a frame alone and as frame two of three


@pytest.mark.parametrize("size", [(9, 33), (8, 32)])
def test_out_at_any_byte_offset_writes_only_the_view(size):
    G = handle()
    model, s, T, B = (32, 32), 4, 2, 2
    a0, b0, f = noise((B,) + size + (3,), 13), noise((B,) + size + (3,), 14), random_field(B, *model, 79, 15)
    ta, tb, tf = dev(G, a0, b0, f)
    want = G.mci_frames_scaled(ta, tb, tf, model, s, k_first=1, count=T)
    assert torch.equal(want.cpu(), torch.from_numpy(host(a0, b0, f, model, s, [1, 2], "clamp", "full")))
    n = want.numel()
    for off in (1, 2, 3):
        buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=G.device)
        view = buf[off:off + n].view(want.shape)
        res = G.mci_frames_scaled(ta, tb, tf, model, s, k_first=1, count=T, out=view)
        assert res.data_ptr() == buf.data_ptr() + off
        assert torch.equal(view, want)
        assert bool((buf[:off] == 0xA5).all()) and bool((buf[off + n:] == 0xA5).all())


def test_the_widest_row_takes_the_unstaged_path():
    """Both widths at 16384: the output row and the blended field row no longer fit 64 KB of LDS together, the field is then
    read from global memory.  One row per frame, equal sizes: the definition and rib_mci_frames agree with it."""
    G = handle()
    model = size = (1, 16384)
    a0, b0, f = noise((1,) + size + (3,), 16), noise((1,) + size + (3,), 17), random_field(1, *model, 79, 18)
    ta, tb, tf = dev(G, a0, b0, f)
    got = G.mci_frames_scaled(ta, tb, tf, model, 4, k_first=1, count=2, border="valid")
    assert torch.equal(got.cpu(), torch.from_numpy(host(a0, b0, f, model, 4, [1, 2], "valid", "full")))
    assert torch.equal(got, G.mci_frames(ta, tb, tf, 4, k_first=1, count=2, normalised=False, border="valid"))
    # 16376 wide on both sides is the widest pair whose field row is still staged: 49152 + 2047 * 8 = 65528 bytes of LDS
    model2 = (1, 16376)
    f2 = random_field(1, *model2, 79, 19)
    (tf2,) = dev(G, f2)
    got2 = G.mci_frames_scaled(ta[:, :, :16376], tb[:, :, :16376], tf2, model2, 4, k_first=1, count=1)
    want2 = host(a0[:, :, :16376], b0[:, :, :16376], f2, model2, 4, [1], "clamp", "full")
    assert torch.equal(got2.cpu(), torch.from_numpy(want2))


def test_refusals_leave_the_output_untouched():
    G = handle()
    L, H_ = G._lib, G._h
    model, size = (32, 32), (40, 48)
    a0, b0, f = noise((1,) + size + (3,), 20), noise((1,) + size + (3,), 21), random_field(1, *model, 79, 22)
    ta, tb, tf = dev(G, a0, b0, f)
    out = torch.full((2, 1) + size + (3,), 0x5A, dtype=torch.uint8, device=G.device)

    def call(T=2, B=1, H=32, W=32, H0=40, W0=48, a=ta, b=tb, fld=tf, s=4, k=1, border=0, precision=0, o=out):
        ptr = lambda t: t.data_ptr() if t is not None else None
        return L.rib_scaled_frames(H_, T, B, H, W, H0, W0, ptr(a), ptr(b), ptr(fld), s, k, border, precision, ptr(o), None)

    bad = [dict(T=0), dict(B=0), dict(H=0), dict(W=16385), dict(H0=0), dict(W0=16385), dict(W0=16 * 32 + 1), dict(H0=1, H=17),
           dict(W0=1), dict(s=3), dict(s=2048), dict(k=4), dict(k=-1), dict(border=2), dict(precision=2), dict(a=None), dict(fld=None),
           dict(o=None)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert L.rib_last_error(H_).startswith(b"rib_scaled_frames"), (kw, L.rib_last_error(H_))
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    # the Python method refuses the same before the entry is reached
    for kw in (dict(model_hw=(32, 2)), dict(model_hw=(32, 32), sample_rate=3), dict(model_hw=(40, 32))):
        args = dict(model_hw=(32, 32), sample_rate=4)
        args.update(kw)
        with pytest.raises(ValueError):
            G.mci_frames_scaled(ta, tb, tf, **args)
    with pytest.raises(ValueError, match="within 1/16"):            # (32, 32) -> (1, 1): the reduction beyond 16
        G.mci_frames_scaled(ta[:, :1, :1], tb[:, :1, :1], tf, (32, 32), 4)
    assert call() == 0                                               # and the good call is accepted
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(host(a0, b0, f, model, 4, [1, 2], "clamp", "full")))


# ---- the folder driver ---------------------------------------------------------------------------------------------------------
def test_native_folder_driver_at_the_key_frames_size(tmp_path, monkeypatch):
    """64x64 model, 80x96 key frames, two clips of 3 key frames at rate 4, batch 2, chunk 2 (first and later chunks, a loose last
    key frame), poses from the folder: the PNGs and the .avi of the native path under output_size="keyframes" are those of the
    reference-protocol path through the same Generator; frames="none" writes the same .avi and no PNG, with threads and with
    worker processes; and the chain's (img, mask) of every unit are those of output_size="model"."""
    import os
    from PIL import Image
    from render_in_between_amd import evaluator as ev, video
    from tests.composite_common import write_example
    from tests.test_gpu_composite import cfg64, tree
    from tests.test_gpu_mci import Protocol
    from tests.test_keyframes_size_cpu import moving_keys
    root = str(tmp_path)
    n = write_example(root, n_key=3, rate=4, key_hw=(80, 96), clip="clipA", seed=1)
    write_example(root, n_key=3, rate=4, key_hw=(80, 96), clip="clipB", seed=2)
    moving_keys(root, 3, (80, 96), clip="clipA", step=(6, -2))
    moving_keys(root, 3, (80, 96), clip="clipB", step=(-4, 4))
    G = handle()
    inputs_dir, pose_dir = os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")
    seen = []
    chain = G.chain

    def recording_chain(*a, **k):               # every unit's images and masks (asked for under either output size)
        k["want_all"] = True
        out = chain(*a, **k)
        seen.append((out[0].clone(), out[1].clone()))
        return out
    monkeypatch.setattr(G, "chain", recording_chain)

    def run(name, io_mode="thread", **kw):
        out = os.path.join(root, name)
        E = ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1, io_mode=io_mode)
        return out, E.evaluate_from_folder(G, inputs_dir, None, pose_dir, out, background="mci", mci_border="valid", **kw)

    kw = dict(output_size="keyframes", video=True, video_quality=85)
    nat, nat_w = run("native", **kw)
    at_keys, seen = seen, []
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        ref = os.path.join(root, "ref")
        ev.Evaluator(cfg64()).evaluate_from_folder(Protocol(G), inputs_dir, None, pose_dir, ref, background="mci", mci_border="valid", **kw)
    finally:
        G.set_plan_batch(before)
    a, b = tree(nat), tree(ref)
    assert sorted(a) == sorted(b) and len(a) == 2 * n + 2 and n == 9
    for name in sorted(a):
        assert a[name] == b[name], name
    assert len(nat_w) == 2 * n and np.asarray(Image.open(nat_w[1])).shape == (80, 96, 3)
    for k in range(3):                          # a key frame is its file's own pixels
        assert np.array_equal(np.asarray(Image.open(nat_w[4 * k])), np.asarray(Image.open(os.path.join(inputs_dir, "clipA", "%04d.png" % k))))
    for io_mode in ("thread", "process"):
        none, none_w = run("none_" + io_mode, io_mode, frames="none", **kw)
        assert sorted(os.listdir(none)) == ["clipA_video.avi", "clipB_video.avi"]
        assert none_w == [video.frame_name(none, c, i) for c in ("clipA", "clipB") for i in range(n)]
        for c in ("clipA", "clipB"):
            assert open(os.path.join(none, c + "_video.avi"), "rb").read() == a[c + "_video.avi"], (io_mode, c)
    seen.clear()
    model, model_w = run("model", video=True, video_quality=85, output_size="model")
    assert np.asarray(Image.open(model_w[1])).shape == (64, 64, 3)
    assert len(seen) == len(at_keys) == 4       # two clips x one group x two chunks
    for (i0, m0), (i1, m1) in zip(at_keys, seen):
        assert torch.equal(i0, i1) and torch.equal(m0, m1)
