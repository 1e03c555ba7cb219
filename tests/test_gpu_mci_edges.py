"""rib_mci_field / rib_mci_frames (csrc/mci.hip.h) on the inputs that reach what tests/test_gpu_mci.py's smooth, slowly moving
textures never do: candidates of equal cost (the packed key's lower fields and its lane reductions), displacements up to
MAX_DISP of both signs (the biased 6-bit fields, windows clamped far outside the frame), frames wider than one pass of
k_mci_frames' strip loop, frames smaller than a block, a level-1 tile or a pyramid tile, more blocks than one pass of
k_mci_median's grid, the end frames k = 0 and k = s and the largest sample rate.  tests/test_background_cpu.py builds the inputs
and shows with the definition alone that they reach those branches.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from render_in_between_amd import background as bg
from tests.mci_gpu_common import dev, ref
from tests.test_background_cpu import (LONG_MOTIONS, LONG_SIZES, TIE_KINDS, TIE_SIZES, TINY_SIZES, WIDE_SIZES, long_pair, moving_pair,
                                       random_pair, texture, tie_pair, wide_pair)
from tests.test_gpu_mci import handle

pytestmark = pytest.mark.gpu


def check_pairs(G, refs, s, ks=None, both=True):
    """The field of a batch of pairs and its frames ks (default: every interior frame, in one launch) against the definition."""
    ks = list(range(1, s)) if ks is None else list(ks)
    ta, tb = dev(G, np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs]))
    field = G.mci_field(ta, tb)
    want_f = np.stack([r[2] for r in refs])
    assert field.dtype == torch.int16 and tuple(field.shape) == want_f.shape
    assert torch.equal(field.cpu(), torch.from_numpy(want_f))
    if not ks:
        return field, None
    want = np.stack([bg.mci_frames_host(r[0], r[1], r[2], s, ks) for r in refs], 1)          # [T, B, H, W, 3]
    runs = [[ks[0]]]                                                    # consecutive k share a launch (k_first, count)
    for k in ks[1:]:
        if k == runs[-1][-1] + 1:
            runs[-1].append(k)
        else:
            runs.append([k])
    got = []
    for run in runs:
        if both:
            f32, u8 = G.mci_frames(ta, tb, field, s, k_first=run[0], count=len(run), normalised="both")
            assert torch.equal(f32.cpu(), torch.from_numpy(bg.normalised_upload(u8.cpu().numpy())))
        else:
            u8 = G.mci_frames(ta, tb, field, s, k_first=run[0], count=len(run), normalised=False)
        got.append(u8)
    got = torch.cat(got)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    return field, got


def tie_ref(kind, h, w):
    return ref(("tie", kind, h, w), lambda: tie_pair(kind, h, w))


def long_ref(h, w, i):
    return ref(("long", h, w, i), lambda: long_pair(h, w, i))


@pytest.mark.parametrize("h,w", TIE_SIZES)
def test_candidates_of_equal_cost(h, w):
    """Periodic patterns against their half-period shift: the winner of most blocks is decided by (|d|^2, dy, dx).  In batches
    of three mixed patterns and alone: a pair's field and frames do not depend on the batch."""
    G = handle()
    refs = [tie_ref(kind, h, w) for kind in TIE_KINDS]
    assert any(r[2].any() for r in refs)
    alone = [check_pairs(G, [r], 4) for r in refs]
    n = len(refs)
    for first in range(0, n, 2):                                        # (0 1 2) (2 3 4) (4 5 6) (6 0 1): mixed patterns
        idx = [(first + j) % n for j in range(3)]
        field, frames = check_pairs(G, [refs[i] for i in idx], 4)
        for j, i in enumerate(idx):
            assert torch.equal(field[j], alone[i][0][0]) and torch.equal(frames[:, j], alone[i][1][:, 0])


@pytest.mark.parametrize("h,w", LONG_SIZES)
def test_displacements_up_to_the_largest(h, w):
    """Motion at and beyond the edge of the search: fields full of +-16..19 in both components."""
    G = handle()
    refs = [long_ref(h, w, i) for i in range(len(LONG_MOTIONS))]
    allf = np.stack([r[2] for r in refs])
    assert np.abs(allf).max() == bg.MAX_DISP and allf.min() == -bg.MAX_DISP
    check_pairs(G, refs, 4)
    for r in refs:
        check_pairs(G, [r], 4, both=False)


def test_the_largest_sample_rate_on_long_vectors():
    G = handle()
    h, w = LONG_SIZES[0]
    check_pairs(G, [long_ref(h, w, 1)], bg.MAX_SAMPLE_RATE, ks=(1, 511, 512, 1023))


def test_end_frames_are_the_key_frames():
    G = handle()
    h, w = 67, 93
    a, b, f = ref(("end", h, w), lambda: moving_pair(h, w, 12, -6, 40))
    assert f.any()
    for s in (8, 1):
        host = bg.mci_frames_host(a, b, f, s, [0, s])
        assert np.array_equal(host[0], a) and np.array_equal(host[1], b)
        _, got = check_pairs(G, [(a, b, f)], s, ks=(0, s))
        assert torch.equal(got[0, 0].cpu(), torch.from_numpy(a)) and torch.equal(got[1, 0].cpu(), torch.from_numpy(b))
    check_pairs(G, [(a, b, f)], 8, ks=range(0, 9))                      # the whole segment in one launch


@pytest.mark.parametrize("h,w", WIDE_SIZES)
def test_frames_wider_than_one_pass_of_the_strip_loop(h, w):
    """W > 1024: a thread of k_mci_frames takes a second (and at 4100 a fifth) strip of four pixels.  Both outputs; then the
    uint8 output into a caller's buffer 1 and 7 bytes into a larger allocation, around which nothing may change."""
    G = handle()
    a, b, f = ref(("wide", h, w), lambda: wide_pair(h, w))
    assert f.any()
    field, u8 = check_pairs(G, [(a, b, f)], 4)
    ta, tb = dev(G, a, b)
    n = 3 * h * w * 3
    for off in (1, 7):
        buf = torch.full((off + n + 64,), 77, dtype=torch.uint8, device=G.device)
        out = buf[off:off + n].view(3, h, w, 3)
        assert out.data_ptr() % 16 == off
        G.mci_frames(ta, tb, field[0], 4, normalised=False, out=out)
        host = buf.cpu()
        assert torch.equal(host[off:off + n].view(3, h, w, 3), u8[:, 0].cpu()), off
        assert (host[:off] == 77).all() and (host[off + n:] == 77).all(), off


@pytest.mark.parametrize("h,w", TINY_SIZES)
def test_frames_smaller_than_a_tile(h, w):
    G = handle()
    r = ref(("tiny", h, w, 1), lambda: random_pair(h, w, 1))
    assert r[2].shape == bg.field_shape(h, w) + (2,)
    check_pairs(G, [r], 2)
    check_pairs(G, [r], bg.MAX_SAMPLE_RATE, ks=(0, 1, 511, 512, 1023, 1024))


def test_a_batch_of_tiny_frames():
    G = handle()
    moved = 0
    for h, w in ((7, 9), (9, 33), (1, 1)):
        refs = [ref(("tiny", h, w, seed), lambda: random_pair(h, w, seed)) for seed in (1, 2)]
        moved += any(r[2].any() for r in refs)
        check_pairs(G, refs, 2)
        check_pairs(G, refs, bg.MAX_SAMPLE_RATE, ks=(1, 1023))
    assert moved


def test_median_over_more_blocks_than_one_pass_of_its_grid():
    """65 frames of 16 x 16384: 266240 blocks, more than the 1024 workgroups of k_mci_median hold in one pass.  Three distinct
    moving pairs in a fixed pattern; the definition computes three fields."""
    G = handle()
    h, w, B = 16, 16384, 65
    tex = texture(h + 12, w + 44, 50)                                   # one scene, three motions (dx, dy)
    crop = lambda dx, dy: np.ascontiguousarray(tex[6 - dy:6 - dy + h, 22 - dx:22 - dx + w])
    three = [ref(("median", i), lambda: (crop(0, 0), crop(*[(14, 2), (-22, -4), (6, 6)][i]))) for i in range(3)]
    assert all(r[2].any() for r in three) and B * three[0][2].shape[0] * three[0][2].shape[1] > 1024 * 256
    pattern = [(i + i // 5) % 3 for i in range(B)]
    ta = torch.stack(dev(G, *[r[0] for r in three]))[pattern]
    tb = torch.stack(dev(G, *[r[1] for r in three]))[pattern]
    field = G.mci_field(ta, tb)
    want = torch.from_numpy(np.stack([r[2] for r in three]))[pattern]
    assert tuple(field.shape) == (B, 2, 2048, 2) and torch.equal(field.cpu(), want)


def test_two_calls_give_equal_tensors():
    G = handle()
    for a, b, _ in (tie_ref("diagonal16", 67, 93), long_ref(96, 160, 1)):
        ta, tb = dev(G, a, b)
        f1, f2 = G.mci_field(ta, tb), G.mci_field(ta, tb)
        assert torch.equal(f1, f2)
        u1, u2 = (G.mci_frames(ta, tb, f1, 4, normalised="both") for _ in range(2))
        assert torch.equal(u1[0], u2[0]) and torch.equal(u1[1], u2[1])
