"""The lossless PNG stream on the host (no GPU): png.encode_host, the definition the GPU encoder (rib_png) is held to - every
fixture of tests/png_common.py decodes pixel-exact in PIL with its chunk CRCs verified, its IDAT data inflate to the filtered
bytes, the size bound holds, the tables are complete, every filter and several tables are exercised, a filter tie goes to the
lower type - and the argument rules of evaluate_from_folder(png_on=...) and of the command line."""
import io
import os
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_common as C

png = C.load_png()
_FILES = {}


def files():
    """{case: ([file per frame], [info per frame])}, encoded once."""
    if not _FILES:
        for name, frames in C.cases():
            infos = [{} for _ in frames]
            _FILES[name] = ([png.encode_host(f, info=i) for f, i in zip(frames, infos)], infos)
    return _FILES


CASES = dict(C.cases())


@pytest.mark.parametrize("name", list(CASES))
def test_every_decoder_reads_the_file(name):
    for img, data in zip(CASES[name], files()[name][0]):
        Image.open(io.BytesIO(data)).verify()                      # the chunk CRCs
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img)
        payload, count = C.idat_payload(data)
        H, W, _ = img.shape
        assert count == 2 + -(-H // png.STRIP_ROWS)                # the zlib header, one chunk per strip, the Adler-32
        assert payload[:2] == b"\x78\x01"
        assert zlib.decompress(payload) == C.filtered_host(png, img)
        assert len(data) <= png.max_bytes(H, W)
        assert data[:47] == png.prefix(H, W) and data[-12:] == png.chunk(b"IEND", b"")


def test_the_tables_are_complete_and_table_0_is_flat():
    T = png.TABLES
    assert T.dtype == np.uint8 and T.ndim == 2 and T.shape[1] == 286 and 1 <= T.shape[0] <= 16
    assert T.min() >= 1 and T.max() <= 15 and T[0].max() <= 9
    for t in T:
        assert sum(2 ** (15 - int(l)) for l in t) == 2 ** 15       # Kraft sum exactly 1
    png.check_tables(T)
    assert png.coder().header_bits.max() <= png.HEADER_BITS_BOUND
    bad = T.copy()
    bad[1, 0] += 1
    with pytest.raises(ValueError, match="complete"):
        png.check_tables(bad)
    bad = T.copy()
    bad[0] = T[1]
    with pytest.raises(ValueError):
        png.check_tables(bad)
    with pytest.raises(ValueError):
        png.check_tables(T[:, :285])


def test_the_generator_script_reproduces_the_committed_tables():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_png_tables", os.path.join(C.ROOT, "tools", "png_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert np.array_equal(np.array(mod.tables(), np.uint8), png.TABLES)


def test_every_filter_and_three_tables_are_chosen():
    filters, tables = set(), set()
    for _, infos in files().values():
        for i in infos:
            filters |= set(int(f) for f in i["filters"])
            tables |= set(i["tables"])
    assert filters == {0, 1, 2, 3, 4}
    assert len(tables) >= 3
    assert 0 in set(files()["24x96-noise"][1][0]["tables"])       # uniform noise: the flat table
    assert len(set(files()["24x300-mixed"][1][0]["tables"])) == 3      # smooth, noisy and flat strips: three tables in one file


def test_the_run_length_frame_holds_the_runs_it_is_named_after():
    for img in CASES["runs"]:
        d = png.filter_rows(img)[0].reshape(-1)
        assert d[0] == 1                                            # Sub
        sym, length = png.strip_tokens(d)
        got = sorted(int(l) for l in length if l)
        # behind its literal a run of 258 + r, r < 4, is one match and r literals; of 262 / 263 a match of 258 and one of 4 / 5
        assert got == sorted([4, 5, 258, 258, 258, 258, 4, 5])
    zero = png.filter_rows(CASES["17x64-zero"][0])[0][:8].reshape(-1)
    sym, length = png.strip_tokens(zero)
    n = zero.size
    assert length.tolist() == [0] + [258] * ((n - 1) // 258) + ([(n - 1) % 258] if (n - 1) % 258 >= 4 else [0] * ((n - 1) % 258))


def test_a_filter_tie_goes_to_the_lower_type():
    """Row 0 of a frame has nothing above it: Up is None and Paeth is Sub there, so two pairs of costs are equal.  With a first
    row whose Sub cost is below its None cost, Sub (1) ties with Paeth (4) and wins; with an alternating row None (0) ties with
    Up (2) and wins."""
    ramp = np.repeat(np.arange(100, 116, dtype=np.uint8)[None, :, None], 3, axis=2)             # [1, 16, 3]
    info = {}
    png.encode_host(ramp, info=info)
    _, costs = png.filter_rows(ramp)
    assert costs[0, 1] == costs[0, 4] == costs[0].min() and info["filters"][0] == 1
    alt = np.zeros((1, 16, 3), np.uint8)
    alt[0, ::2] = 3
    alt[0, 1::2] = 253                                              # |int8| = 3 either way; Sub sees steps of 6
    png.encode_host(alt, info=info)
    _, costs = png.filter_rows(alt)
    assert costs[0, 0] == costs[0, 2] == costs[0].min() and info["filters"][0] == 0
    # constructed row pairs: on the second row Sub and Up tie for the minimum (320) and Sub wins; Up and Paeth tie (135), Up wins
    for rows, tied in (([[[96, 224, 64], [32, 128, 160]], [[64, 192, 0], [160, 128, 224]]], (1, 2)),
                       ([[[0, 9, 27], [36, 63, 54]], [[18, 36, 45], [63, 27, 45]]], (2, 4))):
        pair = np.array(rows, np.uint8)
        _, costs = png.filter_rows(pair)
        assert tuple(f for f in range(5) if costs[1, f] == costs[1].min()) == tied
        png.encode_host(pair, info=info)
        assert info["filters"][1] == tied[0]


def test_max_bytes_is_a_function_of_the_size_only():
    assert png.max_bytes(1, 1) == 47 + 16 + 12 + png.strip_bound(4)
    assert png.max_bytes(9, 5) == 47 + 16 + 12 + png.strip_bound(8 * 16) + png.strip_bound(16)
    for bad in ((0, 1), (1, 0), (65536, 1), (1, 4097)):
        with pytest.raises(ValueError):
            png.max_bytes(*bad)
    with pytest.raises(ValueError):
        png.encode_host(np.zeros((4, 4), np.uint8))


def test_argument_errors_of_the_folder_driver(tmp_path):
    from render_in_between_amd import evaluator as ev
    from tests.test_driver import _write_example, oracle_labels
    from tests.test_panels_cpu import Recorder, small_cfg
    root = str(tmp_path)
    _write_example(root, n_key=2, rate=2)
    cfg = small_cfg()
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    out = os.path.join(root, "o")

    class Native(Recorder):                      # enough of the native surface to get past the protocol check
        chain = quantise = png_into = None

    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    with pytest.raises(ValueError, match="png_on"):
        E.evaluate_from_folder(Recorder(cfg), *dirs, out, png_on="device")
    with pytest.raises(ValueError, match="reference's protocol"):
        E.evaluate_from_folder(Recorder(cfg), *dirs, out, png_on="gpu")
    with pytest.raises(ValueError, match="frames="):
        E.evaluate_from_folder(Native(cfg), *dirs, out, png_on="gpu", video=True, frames="none")
    with pytest.raises(ValueError, match="PNG level"):
        ev.Evaluator(cfg, label_fn=oracle_labels, png_compress_level=1).evaluate_from_folder(Native(cfg), *dirs, out, png_on="gpu")
    assert not os.path.exists(out)


def test_command_line_flag_reaches_the_driver(monkeypatch):
    from render_in_between_amd import inference
    assert inference.parse_args(["--input-dir", "x"]).png_on == "host"
    o = inference.parse_args(["--input-dir", "x", "--png-on", "gpu"])
    assert o.png_on == "gpu"
    for bad in (["--png-on", "gpu", "--png-level", "1"], ["--png-on", "gpu", "--video", "--frames", "none"], ["--png-on", "cpu"]):
        with pytest.raises(SystemExit):
            inference.parse_args(["--input-dir", "x"] + bad)
    seen = {}

    class Stop(Exception):
        pass

    def fake(self, model, *a, **kw):
        seen.update(kw)
        raise Stop
    monkeypatch.setattr(inference, "load_generator", lambda *a, **k: object())
    monkeypatch.setattr(inference.rib, "get_config", lambda path: inference.rib.AttrDict(model_height=32, model_width=48, gauss_sigma=5,
                                                                                         skeleton_thres=0.001, foot_thres=0.001))
    monkeypatch.setattr(inference.Evaluator, "evaluate_from_folder", fake)
    with pytest.raises(Stop):
        inference.main(o)
    assert seen["png_on"] == "gpu"
    seen.clear()
    with pytest.raises(Stop):
        inference.main(inference.parse_args(["--input-dir", "x"]))
    assert seen["png_on"] == "host"
