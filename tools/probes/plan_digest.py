"""Launch plans, field for field, on host-only handles: one line per plan over shapes x precision x products x plan flags x
taps x Winograd input staging x policy switches x tuned choices, and the refusals of the tuned-choice lookups.  CPU only.

Needs a librib.so with the debug entry of tools/probes/plan_digest.patch (`git apply`, then csrc/build.py; the entry is not
part of the library as committed).  Two trees plan alike when their outputs are byte-identical:

    python tools/probes/plan_digest.py --out new.txt
    RIB_LIBRARY=<other tree>/render-in-between_amd/csrc/librib.so python tools/probes/plan_digest.py --out parent.txt
    cmp parent.txt new.txt && sha256sum parent.txt new.txt

Switches that are read once per process (RIB_NO_DMA, RIB_NO_XCD) need a process of their own, so every environment runs in a
child of this script."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

EXTRA_SHAPES = ((1, 512, 512), (4, 512, 512), (1, 320, 480), (3, 96, 160), (1, 1024, 1024))
PLAN_LABELS, PLAN_UNPAIRED = 1, 2
DTYPES = (("f32", 0), ("bf16", 1), ("f16", 3))      # name, RIB_DTYPE_*


def environments():
    from tests import policy_common as pc
    from tests.test_policy_cpu import HELD_ELSEWHERE
    envs = [{}]
    for c in pc.CASES:
        for e in (c.env, c.base):
            if "largest" in e.values():      # the row's placeholder: both sides of an inclusive threshold
                envs += [{k: "1024" for k in e}, {k: "1023" for k in e}]
            elif e:
                envs.append(dict(e))
    values = {"RIB_WINO_M": ("2", "4"), "RIB_WINO_SHORTCUT_M": ("2", "4"), "RIB_LOWC_TW": ("16", "32")}
    for k in sorted(HELD_ELSEWHERE):
        envs += [{k: v} for v in values.get(k, ("1",))]
    out = []
    for e in envs:
        if e not in out:
            out.append(e)
    return out, pc


def shapes_of(pc):
    return tuple(pc.SHAPES) + (pc.XCD_SHAPE,) + EXTRA_SHAPES


class Handle:
    def __init__(self, lib, dtype):
        import render_in_between_amd as rib
        from render_in_between_amd import _native
        spec = rib.GenSpec.from_cfg(rib.hsm_gen_config())
        c = _native.RibConfig(**{n: getattr(spec, n) for n, _ in _native.RibConfig._fields_})
        self.lib, self.h = lib, C.c_void_p()
        assert lib.rib_create(C.byref(c), -1, C.byref(self.h)) == 0, lib.rib_last_error(None)
        assert lib.rib_set_compute_dtype(self.h, dtype) == 0
        self.buf = C.create_string_buffer(400)

    def digest(self, B, H, W, flags, tuneB):
        rc = self.lib.rib_debug_plan_digest(self.h, B, H, W, flags, tuneB, self.buf, 400)
        return self.buf.value.decode() if rc == 0 else "rc=%d %s" % (rc, self.lib.rib_last_error(self.h).decode())

    def launches(self, B, H, W):
        buf = C.create_string_buffer(600)
        out = []
        for i in range(self.lib.rib_num_launches(self.h, B, H, W)):
            assert self.lib.rib_debug_launch_info(self.h, B, H, W, i, buf, 600) == 0
            out.append(buf.value.decode().split("|")[0])
        return out

    def close(self):
        self.lib.rib_destroy(self.h)


def plans_of(shape, chain_t):
    """(flags, batch, tuneB) of the plans a frame, a chain and its labels-only pre-pass ask for."""
    B = shape[0]
    return ((0, B, 0), (PLAN_UNPAIRED, B, 0), (PLAN_LABELS, B, 0), (PLAN_LABELS, chain_t * B, 1), (PLAN_LABELS, chain_t * B, B))


def variants(lib):
    g = (C.c_int * 12)()
    out = []
    for i in range(lib.rib_num_variants()):
        prec = lib.rib_variant_info(i, g)
        out.append(dict(zip("FRW WM WN MF NF BK STRIDE KS UPS SPADE KW TB".split(), g), prec=prec, idx=i))
    return out


def refusals(lib, say):
    """One tuned choice that does not fit per lookup site, and one that does for the fused-shortcut Winograd switch-over."""
    vs = variants(lib)
    first = lambda **kw: next(v["idx"] for v in vs if all(v[k] == x for k, x in kw.items()))
    spade32 = first(prec=0, SPADE=1, NF=2, KW=1, TB=1)
    one32 = first(prec=0, SPADE=0, KS=1, STRIDE=1, UPS=0, NF=2, KW=1, TB=1, BK=32)
    one16 = first(prec=1, SPADE=0, KS=1, STRIDE=1, UPS=0, NF=2, KW=1)
    dma32 = first(prec=0, FRW=0)
    B, H, W = 1, 64, 64
    h = Handle(lib, 0)
    names = h.launches(B, H, W)
    h.close()
    wino = next(n for n in names if n.endswith((".wino", ".wino4")))
    level = next(n for n in names if n.endswith(".gammabeta"))
    cases = (("conv", "ref_embedding.down_0", spade32, 1), ("wino_gemm", wino, one32, 2), ("cond_level_gemm", level, one16, 1),
             ("spade", "down_0.0.spade", one16, 1), ("spade_dma", "down_0.0.spade", dma32, 1),
             ("shortcut_wino_igemm", "down_1.conv_block_1.wino", one32, 1), ("shortcut_wino4_igemm", "down_1.conv_block_1.wino4", one32, 1),
             ("shortcut_wino_dma", "down_1.conv_block_1.wino", dma32, 1), ("shortcut_wino4_dma", "down_1.conv_block_1.wino4", dma32, 1))
    for what, op, idx, ks in cases:
        for cond0 in (False, True):      # the SPADE's own lookup decides only without the level GEMM
            if cond0:
                os.environ["RIB_COND_GEMM_MAX_PX"] = "0"
            h = Handle(lib, 0)
            rc = lib.rib_set_choice(h.h, B, H, W, op.encode(), idx, ks)
            say("refusal %s cond0=%d op=%s variant=%d ksplit=%d set=%d -> %s" % (what, cond0, op, idx, ks, rc, h.digest(B, H, W, 0, 0)))
            h.close()
            os.environ.pop("RIB_COND_GEMM_MAX_PX", None)


def child(env):
    from render_in_between_amd import _native, tuning
    from tests import policy_common as pc
    lib = _native.lib()
    lib.rib_debug_plan_digest.restype = C.c_int
    lib.rib_debug_plan_digest.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    tag = ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"
    say = lambda s: print("%s | %s" % (tag, s))
    shapes = shapes_of(pc)
    for dname, dtype in DTYPES:
        for tuned in (False, True):
            table = tuning.load(dtype=dname) if tuned else {}
            todo = shapes + tuple(tuple(int(x) for x in k.split(",")) for k in sorted(table) if tuple(int(x) for x in k.split(",")) not in shapes)
            h = Handle(lib, dtype)
            applied = set()
            for products in (0, 1):
                assert lib.rib_set_products(h.h, products) == 0
                for taps in (0, 1):
                    assert lib.rib_set_debug_taps(h.h, taps) == 0
                    for staging in (1, 0):
                        assert lib.rib_set_wino_in_staging(h.h, staging) == 0
                        for shape in todo:
                            B, H, W = shape
                            if tuned and not any("%d,%d,%d" % (b, H, W) in table for b in (1, B)):
                                continue
                            for flags, batch, tuneB in plans_of(shape, pc.CHAIN_T):
                                follow = (tuneB or batch, H, W)
                                if tuned and follow not in applied:      # as Generator._workspace pins them: once per followed shape
                                    applied.add(follow)
                                    n = tuning.apply(lib, h.h, table, *follow, dtype=dname)
                                    say("%s tuned apply %d,%d,%d -> %d" % ((dname,) + follow + (n,)))
                                say("%s tuned=%d products=%d taps=%d staging=%d shape=%d,%d,%d flags=%d batch=%d tuneB=%d -> %s"
                                    % (dname, tuned, products, taps, staging, B, H, W, flags, batch, tuneB, h.digest(batch, H, W, flags, tuneB)))
            h.close()
    if not env:
        refusals(lib, say)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    if a.child is not None:
        import warnings
        warnings.simplefilter("ignore")
        child(json.loads(a.child))
        return
    envs, pc = environments()

    def run(e):
        env = {k: v for k, v in os.environ.items() if k not in pc.POLICY_VARS}
        env.update(e)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(e)], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("child %r failed:\n%s" % (e, r.stderr[-2000:]))
        return r.stdout
    with ThreadPoolExecutor(a.jobs) as ex:
        text = "".join(ex.map(run, envs))
    with (open(a.out, "w") if a.out else sys.stdout) as f:
        f.write(text)
    print("%d rows, %d environments" % (text.count("\n"), len(envs)), file=sys.stderr)


if __name__ == "__main__":
    main()
