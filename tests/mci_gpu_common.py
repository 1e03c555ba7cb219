"""What tests/test_gpu_mci_edges.py, test_gpu_mci_range.py and test_gpu_mci_border.py share: the inputs and their fields by the
definition (background.mci_field_host), each made once, and the exact comparison of Generator.mci_field with them."""
import numpy as np
import torch

from render_in_between_amd import background as bg

_PAIRS, _REF = {}, {}


def ref(key, make, levels=3, border="clamp"):
    """(a, b, field) of the definition: the input `key` is built once (make() -> (a, b)), its field once per (levels, border)."""
    if key not in _PAIRS:
        _PAIRS[key] = tuple(make())
    if (key, levels, border) not in _REF:
        _REF[key, levels, border] = _PAIRS[key] + (bg.mci_field_host(*_PAIRS[key], levels, border),)
    return _REF[key, levels, border]


def dev(G, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(G.device) for x in arrays)


def check_field(G, refs, levels, border="clamp"):
    """The field of a batch of refs in one call against the definition's, exactly -> the device field."""
    ta, tb = dev(G, np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs]))
    field = G.mci_field(ta, tb, levels, border=border)
    want = np.stack([r[2] for r in refs])
    assert field.dtype == torch.int16 and tuple(field.shape) == want.shape
    assert torch.equal(field.cpu(), torch.from_numpy(want)), (levels, border, refs[0][0].shape)
    return field


def check_defaults(G, a, b, levels=3, s=4):
    """levels = 3 and border = 0 ("clamp") are the defaults: the raw C entries with border = 0, the Generator's methods without
    the argument and with border="clamp" (at levels = 3 also without levels) give one field and one set of frames k = 0..s in
    both outputs, byte for byte - the definition's; the size query is positive and grows with every level."""
    L = G._lib
    h, w = a.shape[:2]
    ta, tb = dev(G, a, b)
    sizes = [L.rib_mci_workspace_bytes(G._h, 1, h, w, n) for n in (3, 4, 5)]
    assert 0 < sizes[0] < sizes[1] < sizes[2]
    ws = torch.empty(sizes[levels - 3], dtype=torch.uint8, device=G.device)
    raw = torch.full(bg.field_shape(h, w) + (2,), 77, dtype=torch.int16, device=G.device)
    assert L.rib_mci_field(G._h, 1, h, w, ta.data_ptr(), tb.data_ptr(), raw.data_ptr(), levels, 0, ws.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(G.mci_field(ta, tb, levels), raw) and torch.equal(G.mci_field(ta, tb, levels, border="clamp"), raw)
    if levels == 3:
        assert torch.equal(G.mci_field(ta, tb), raw)
    assert torch.equal(raw.cpu(), torch.from_numpy(bg.mci_field_host(a, b, levels)))
    T = s + 1
    f32 = torch.full((T, 1, 3, h, w), 7.0, device=G.device)
    u8 = torch.full((T, 1, h, w, 3), 9, dtype=torch.uint8, device=G.device)
    assert L.rib_mci_frames(G._h, T, 1, h, w, ta.data_ptr(), tb.data_ptr(), raw.data_ptr(), s, 0, 0, f32.data_ptr(), u8.data_ptr(), None) == 0
    torch.cuda.synchronize()
    for kw in ({}, {"border": "clamp"}):
        gf, gu = G.mci_frames(ta, tb, raw, s, k_first=0, count=T, normalised="both", **kw)
        assert torch.equal(gf, f32[:, 0]) and torch.equal(gu, u8[:, 0])
    want = bg.mci_frames_host(a, b, raw.cpu().numpy(), s, range(T))
    assert torch.equal(u8[:, 0].cpu(), torch.from_numpy(want)) and torch.equal(f32[:, 0].cpu(), torch.from_numpy(bg.normalised_upload(want)))
