"""The source-size composite on the MI355X: rib_composite (csrc/composite.hip.h, Generator.composite) against its definition
(composite.composite_host) bit for bit - enlargement, reduction on one axis, equal sizes, a strong reduction (the plain path)
and a one-pixel output -, its invariances (batch position, byte offsets of every operand, in place), the composition of the
existing entries it replaces, the refusals of the C entry, and the folder driver's output_size="source" on the native path
against the reference-protocol path.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import composite, evaluator as ev, video
from tests.composite_common import inputs, write_example
from tests.test_gpu_quality import handle

pytestmark = pytest.mark.gpu

# both axes up, no multiple of any tile | one axis down (its tiles' patches exceed the staged rows) | one down, one up, by a
# pixel | x8 with a one-pixel last tile | equal sizes | a strong reduction (the plain path) | a single output pixel
PAIRS = [((64, 64), (136, 240)), ((64, 64), (48, 100)), ((32, 32), (31, 33)), ((32, 32), (130, 257)), ((64, 64), (64, 64)),
         ((64, 96), (7, 9)), ((32, 32), (1, 1))]
_WANT = {}


def want(hw, hw0):
    """The definition's frames of inputs(hw, hw0), computed once."""
    if (hw, hw0) not in _WANT:
        _WANT[(hw, hw0)] = composite.composite_host(*inputs(*hw, *hw0))
    return _WANT[(hw, hw0)]


def dev(hw, hw0):
    return tuple(torch.from_numpy(a).cuda() for a in inputs(*hw, *hw0))


@pytest.mark.parametrize("hw,hw0", PAIRS)
def test_composite_equals_the_definition(hw, hw0):
    G = handle()
    pred, mask, bg = dev(hw, hw0)
    before = bg.clone()
    got = G.composite(pred, mask, bg)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(bg.shape) and got.data_ptr() != bg.data_ptr()
    assert np.array_equal(got.cpu().numpy(), want(hw, hw0))
    assert torch.equal(bg, before)
    # 16-bit predictions and masks are converted first: the definition of their float32 values
    p16, m16 = pred.to(torch.bfloat16), mask.to(torch.float16)
    assert np.array_equal(G.composite(p16, m16, bg).cpu().numpy(),
                          composite.composite_host(p16.float().cpu().numpy(), m16.float().cpu().numpy(), inputs(*hw, *hw0)[2]))


@pytest.mark.parametrize("hw,hw0", [PAIRS[0], PAIRS[1]])
def test_a_frame_alone_and_as_frame_two_of_three(hw, hw0):
    G = handle()
    pred, mask, bg = dev(hw, hw0)
    order = [1, 0, 1]
    three = G.composite(pred[order].contiguous(), mask[order].contiguous(), bg[order].contiguous())
    alone = G.composite(pred[0:1].contiguous(), mask[0:1].contiguous(), bg[0:1].contiguous())
    assert torch.equal(three[1], alone[0]) and np.array_equal(alone[0].cpu().numpy(), want(hw, hw0)[0])


@pytest.mark.parametrize("hw,hw0", [PAIRS[0], PAIRS[1], PAIRS[3]])
def test_byte_offsets_of_every_operand_and_in_place(hw, hw0):
    G = handle()
    pred, mask, bg = dev(hw, hw0)
    ref = want(hw, hw0)
    nbytes = bg.numel()
    for off in (1, 2, 3):                      # out (and bg) 1, 2, 3 bytes into an allocation: nothing outside the view is written
        buf = torch.full((nbytes + 64,), 77, dtype=torch.uint8, device="cuda")
        out = buf[off:off + nbytes].view(bg.shape)
        assert out.data_ptr() % 4 == off
        assert G.composite(pred, mask, bg, out=out) is out
        host = buf.cpu().numpy()
        assert np.array_equal(host[off:off + nbytes].reshape(ref.shape), ref), off
        assert (host[:off] == 77).all() and (host[off + nbytes:] == 77).all(), off
        src = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")[off:off + nbytes].view(bg.shape)
        src.copy_(bg)
        assert np.array_equal(G.composite(pred, mask, src).cpu().numpy(), ref), off
    for off in (1, 2, 3):                      # pred / mask 4, 8, 12 bytes into an allocation
        p = torch.zeros(pred.numel() + off, dtype=torch.float32, device="cuda")[off:].view(pred.shape)
        m = torch.zeros(mask.numel() + off, dtype=torch.float32, device="cuda")[off:].view(mask.shape)
        p.copy_(pred); m.copy_(mask)
        assert p.data_ptr() % 16 == 4 * off and m.data_ptr() % 16 == 4 * off
        assert np.array_equal(G.composite(p, m, bg).cpu().numpy(), ref), off
    inplace = bg.clone()
    assert G.composite(pred, mask, inplace, out=inplace) is inplace
    assert np.array_equal(inplace.cpu().numpy(), ref)


@pytest.mark.parametrize("hw,hw0", PAIRS[:6])
def test_composite_equals_the_composition_of_the_existing_entries(hw, hw0):
    """quantise, the mask to uint8 on three channels, two resize_u8 launches and an integer blend in torch."""
    G = handle()
    pred, mask, bg = dev(hw, hw0)
    (H0, W0) = hw0
    P = G.quantise(pred)
    M = (mask.double().clamp(0, 1) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).expand(-1, -1, -1, 3).contiguous()
    Pu, Mu = G.resize_u8(P, W0, H0).int(), G.resize_u8(M, W0, H0).int()
    blend = ((Pu * Mu + bg.int() * (255 - Mu) + 127) // 255).to(torch.uint8)
    assert torch.equal(G.composite(pred, mask, bg), blend)


def test_bad_arguments_launch_nothing():
    import ctypes as C
    from render_in_between_amd import _native
    G = handle()
    hw, hw0 = PAIRS[2]
    pred, mask, bg = dev(hw, hw0)
    out = torch.full_like(bg, 77)
    for bad in (dict(pred=pred[:, :2]), dict(pred=pred.double()), dict(pred=pred.cpu()), dict(mask=mask[:1]), dict(mask=mask[:, :, :-1]),
                dict(mask=mask.expand(-1, 3, -1, -1)), dict(bg_u8=bg.float()), dict(bg_u8=bg[..., :2]), dict(bg_u8=bg[:1]), dict(bg_u8=bg.cpu()),
                dict(out=out[:1]), dict(out=out.float()), dict(out=out.transpose(1, 2)), dict(out=out.cpu())):
        with pytest.raises(ValueError):
            G.composite(**dict(dict(pred=pred, mask=mask, bg_u8=bg, out=out), **bad))
    L = _native.lib()
    (H, W), (H0, W0) = hw, hw0
    G.composite(pred, mask, bg)                                    # (the tap tables of this size pair exist now)
    tabs = [t.value for t in G._cubic_tables(H, W, H0, W0)]
    ok = [2, H, W, H0, W0, pred.data_ptr(), mask.data_ptr(), bg.data_ptr()] + tabs + [out.data_ptr()]
    torch.cuda.synchronize()
    for i, bad in ((0, 0), (0, 65536), (0, -1), (1, 0), (2, 0), (3, 0), (4, -5), (5, None), (5, pred.data_ptr() + 2), (6, None), (6, mask.data_ptr() + 1),
                   (7, None), (8, None), (9, None), (10, None), (11, None), (12, None)):
        args = list(ok)
        args[i] = bad
        assert L.rib_composite(G._h, *args, None) == -1, (i, bad)       # RIB_ERR_INVALID
        assert b"rib_composite" in L.rib_last_error(G._h), (i, bad)
    torch.cuda.synchronize()
    assert (out == 77).all()


# ---- the folder driver ---------------------------------------------------------------------------------------------------------
def cfg64():
    return rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)


def tree(out):
    return {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(out) for f in fs}


def test_native_folder_driver_at_the_source_size(tmp_path):
    """64x64 model, 96x80 DAIN frames, two clips of 3 key frames at rate 4, batch 2, chunk 2 (first and later chunks, a loose last
    key frame; clipB's key frames are 90x70 files): the PNGs and the .avi of the native path under resize_on="gpu" are those of
    the reference-protocol path through the same Generator; frames="none" writes the same .avi and no PNG, with threads and with
    worker processes; and the default output size writes what a call without the argument writes."""
    from PIL import Image
    from tests.test_gpu_mci import Protocol
    root = str(tmp_path)
    n = write_example(root, n_key=3, rate=4, key_hw=(80, 96), dain_hw=(80, 96), clip="clipA", seed=1)
    write_example(root, n_key=3, rate=4, key_hw=(70, 90), dain_hw=(80, 96), clip="clipB", seed=2)
    G = handle()
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]

    def run(name, io_mode="thread", **kw):
        out = os.path.join(root, name)
        E = ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1, io_mode=io_mode, resize_on="gpu")
        return out, E.evaluate_from_folder(G, *dirs, out, **kw)

    kw = dict(output_size="source", video=True, video_quality=85)
    nat, nat_w = run("native", **kw)
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        ref = os.path.join(root, "ref")
        ev.Evaluator(cfg64()).evaluate_from_folder(Protocol(G), *dirs, ref, **kw)
    finally:
        G.set_plan_batch(before)
    a, b = tree(nat), tree(ref)
    assert sorted(a) == sorted(b) and len(a) == 2 * n + 2 and n == 9
    for name in sorted(a):
        assert a[name] == b[name], name
    assert len(nat_w) == 2 * n and np.asarray(Image.open(nat_w[1])).shape == (80, 96, 3)
    for io_mode in ("thread", "process"):
        none, none_w = run("none_" + io_mode, io_mode, frames="none", **kw)
        assert sorted(os.listdir(none)) == ["clipA_video.avi", "clipB_video.avi"]
        assert none_w == [video.frame_name(none, c, i) for c in ("clipA", "clipB") for i in range(n)]
        for c in ("clipA", "clipB"):
            assert open(os.path.join(none, c + "_video.avi"), "rb").read() == a[c + "_video.avi"], (io_mode, c)
    proc, _ = run("process_png", "process", **kw)
    assert tree(proc) == a
    plain, _ = run("plain", video=True, video_quality=85)
    model, _ = run("model", video=True, video_quality=85, output_size="model")
    assert tree(plain) == tree(model) and np.asarray(Image.open(os.path.join(plain, "clipA", "f001.png"))).shape == (64, 64, 3)
