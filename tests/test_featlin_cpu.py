"""The sparse first layer (ops.feature_plan / FeaturePlan.linear, rlap_feature_plan_build / _apply) without a GPU:

  * the rules -- the host mirror (tests/csrc/featlin_mirror.cc, every value from rlap_amd/csrc/rlap_featlin.h, contraction off)
    against a numpy restatement of the header's prose in sequential np.float64 scalar operations, bit for bit: lists, offsets,
    directories, forward and transposed values;
  * the mirror against the dense float64 products within tests/test_gpu_propagate.py's bound;
  * the mirror in a stand-alone program under -fsanitize=address,undefined, truncated and altered buffers included;
  * the Python -> C mapping on a stub library, every ValueError before the device is touched, the size query on the real library
    (host arithmetic), the exports and the layout of both structures against the header;
  * ops.feature_masks against adapters.drop_feature under equal seeds.

Bound.  |y - ref| <= bound_factor(T, True) * A, with A the sum of the absolute terms and T the number of terms of the longest sum:
the longest list for the forward call, K times the longest list for the transposed call (K view sums are added).  A float32 result
adds its one rounding, 2^-24 (|ref| + bound).  Elements whose terms hold a NaN are compared as NaN on both sides.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import featlin_mirror as fm
from test_gpu_propagate import bound_factor
from util import StubLib, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 256


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return fm.build(tmp_path_factory.mktemp("featlin"))


# ------------------------------------------------------------------------------------------------ the prose, restated
def prose_lists(x):
    """Forward and transposed lists of (other id, coefficient) by the header's prose: kept iff (double)x != 0.0."""
    N, Fin = x.shape
    xd = x.astype(np.float64)
    fwd = [[(j, xd[i, j]) for j in range(Fin) if xd[i, j] != 0.0] for i in range(N)]
    tr = [[(i, xd[i, j]) for i in range(N) if xd[i, j] != 0.0] for j in range(Fin)]
    return fwd, tr


def prose_parts(lists, nnz):
    off, c, ids, dslot, dk = [0], [], [], [], []
    for slot, lst in enumerate(lists):
        off.append(off[-1] + len(lst))
        ids += [e[0] for e in lst]
        c += [e[1] for e in lst]
        if len(lst) > CHUNK:
            for k in range((len(lst) + CHUNK - 1) // CHUNK):
                dslot.append(slot)
                dk.append(k)
    return {"off": np.array(off, dtype=np.int64), "c": np.array(c, dtype=np.float64), "id": np.array(ids, dtype=np.int32),
            "zero": np.zeros(nnz, dtype=np.int32), "dir_slot": np.array(dslot, dtype=np.int64), "dir_k": np.array(dk, dtype=np.int64)}


def prose_forward(fwd, w, keep, K):
    N, F = len(fwd), w.shape[1]
    y = np.zeros((K, N, F), dtype=w.dtype)
    with np.errstate(all="ignore"):
        for k in range(K):
            for i, lst in enumerate(fwd):
                for f in range(F):
                    total = np.float64(0.0)
                    for c0 in range(0, len(lst), CHUNK):
                        acc = np.float64(0.0)
                        for j, c in lst[c0:c0 + CHUNK]:
                            if keep is None or keep[k, j] != 0:
                                t = np.float64(c) * np.float64(w[j, f])
                                acc = acc + t
                        total = total + acc
                    y[k, i, f] = w.dtype.type(total)
    return y


def prose_transposed(tr, g, keep, K):
    Fin, F = len(tr), g.shape[2]
    dw = np.zeros((Fin, F), dtype=g.dtype)
    with np.errstate(all="ignore"):
        for j, lst in enumerate(tr):
            for f in range(F):
                total = np.float64(0.0)
                for k in range(K):
                    if keep is not None and keep[k, j] == 0:
                        continue
                    s = np.float64(0.0)
                    for c0 in range(0, len(lst), CHUNK):
                        acc = np.float64(0.0)
                        for i, c in lst[c0:c0 + CHUNK]:
                            t = np.float64(c) * np.float64(g[k, i, f])
                            acc = acc + t
                        s = s + acc
                    total = total + s
                dw[j, f] = g.dtype.type(total)
    return dw


@pytest.fixture(scope="module")
def crafted(mirror):
    """The crafted matrix (with its -0.0, denormal and NaN), its prose lists and the mirror's plan, computed once."""
    out = {}
    for dt in (np.float32, np.float64):
        x = fm.crafted_with_nan(dt)
        fwd, tr = prose_lists(x)
        out[dt] = {"x": x, "fwd": fwd, "tr": tr, "plan": fm.plan(mirror, x)}
    return out


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_lists_offsets_and_directories_against_the_prose(mirror, crafted, dt):
    c = crafted[dt]
    x, p = c["x"], c["plan"]
    assert sorted(set(len(l) for l in c["fwd"][:6])) == sorted(fm.LENGTHS) and sorted(set(len(l) for l in c["tr"][:6])) == sorted(fm.LENGTHS)
    nnz = sum(len(l) for l in c["fwd"])
    assert nnz == p["desc"]["nnz"] == fm.count(mirror, x) == sum(len(l) for l in c["tr"])
    assert np.signbit(x[0, 1]) and x[0, 1] == 0 and len(c["fwd"][0]) == 0                    # -0.0 is dropped
    assert any(np.isnan(e[1]) for e in c["fwd"][4]) and any(0 < abs(e[1]) < np.finfo(np.float32).tiny for e in c["fwd"][5])
    dec = fm.decode(p["buffer"], p["desc"])
    assert fm.same_parts(dec, {"forward": prose_parts(c["fwd"], nnz), "transposed": prose_parts(c["tr"], nnz)})
    assert p["desc"]["chunks_forward"] == p["desc"]["chunks_transposed"] == 2 + 3              # the lists of 257 and 513
    assert p["info"] == {"longest_forward": 513, "longest_transposed": 513, "long_lists_forward": 2, "long_lists_transposed": 2}
    lay = fm.layout(mirror, 520, 520, nnz)
    assert all(lay[k] == p["desc"][k] for k in lay if k != "bytes") and lay["bytes"] == p["desc"]["plan_bytes"] == p["buffer"].size
    assert all(v % 256 == 0 for v in lay.values())
    for d in ("forward", "transposed"):                                                       # one direction: the same parts, alone
        one = fm.plan(mirror, x, d)
        assert fm.same_parts(fm.decode(one["buffer"], one["desc"]), {d: dec[d]}) and one["buffer"].size < p["buffer"].size


@pytest.mark.parametrize("K", [1, 2, 3, 9])
@pytest.mark.parametrize("kind", ["all", "none", "chunk", "random"])
def test_values_against_the_prose(mirror, crafted, K, kind):
    rng = np.random.default_rng(K)
    for dt, F in ((np.float32, 3), (np.float64, 2)):
        c = crafted[dt]
        keep = fm.masks(kind, K, c["x"], seed=K)
        w = rng.uniform(-1, 1, size=(520, F)).astype(dt)
        g = rng.uniform(-1, 1, size=(K, 520, F)).astype(dt)
        y = fm.apply(mirror, c["plan"], w, keep)
        assert fm.same_bits(y, prose_forward(c["fwd"], w, keep, K))
        dw = fm.apply(mirror, c["plan"], g, keep, transpose=True)
        assert fm.same_bits(dw, prose_transposed(c["tr"], g, keep, K))
        if kind == "none":
            assert not y.any() and not dw.any() and not np.signbit(y).any() and not np.signbit(dw).any()
        assert not y[:, 0].any() and not np.signbit(y[:, 0]).any()                            # an empty list: exactly +0.0
        if kind == "chunk":                                                                   # view 0 of the longest row: its first chunk adds nothing
            assert np.isfinite(y[0, 5]).all()
    if K == 1:                                                                                # without masks: K = 1, everything kept
        c = crafted[np.float32]
        w = rng.uniform(-1, 1, size=(520, 3)).astype(np.float32)
        assert fm.same_bits(fm.apply(mirror, c["plan"], w), prose_forward(c["fwd"], w, None, 1))
        assert fm.same_bits(fm.apply(mirror, c["plan"], w), fm.apply(mirror, c["plan"], w, fm.masks("all", 1, c["x"])))


def test_mixed_types_and_small_shapes_against_the_prose(mirror):
    rng = np.random.default_rng(11)
    for N, Fin in ((1, 1), (3, 7), (65, 5)):
        for xdt in (np.float32, np.float64):
            x = fm.random_sparse(N, Fin, 4, xdt, seed=N)
            fwd, tr = prose_lists(x)
            p = fm.plan(mirror, x)
            for wdt in (np.float32, np.float64):
                keep = fm.masks("random", 3, x)
                w = rng.uniform(-1, 1, size=(Fin, 4)).astype(wdt)
                g = rng.uniform(-1, 1, size=(3, N, 4)).astype(wdt)
                assert fm.same_bits(fm.apply(mirror, p, w, keep), prose_forward(fwd, w, keep, 3))
                assert fm.same_bits(fm.apply(mirror, p, g, keep, transpose=True), prose_transposed(tr, g, keep, 3))


# ------------------------------------------------------------------------------------------------ against the dense products
@pytest.mark.parametrize("K", [1, 2, 9])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_against_the_dense_float64_products(mirror, K, dt):
    x = fm.crafted(dt)                                                                        # (no NaN: the bound is about finite sums)
    p = fm.plan(mirror, x)
    rng = np.random.default_rng(K + 40)
    for kind in ("all", "chunk", "random"):
        keep = fm.masks(kind, K, x, seed=K)
        w = rng.uniform(-1, 1, size=(520, 5)).astype(dt)
        g = rng.uniform(-1, 1, size=(K, 520, 5)).astype(dt)
        for transpose, operand, terms in ((False, w, 513), (True, g, 513 * K)):
            out = fm.apply(mirror, p, operand, keep, transpose=transpose)
            ref, A = fm.reference(x, operand, keep, transpose)
            ok, worst = fm.within_bound(out, ref, A, bound_factor(terms, True))
            print(f"{dt.__name__} K={K} {kind} transpose={transpose}: worst |y - ref| / bound = {worst:.3e}")
            assert ok, (kind, transpose, worst)
            assert (out[A == 0] == 0).all()


# ------------------------------------------------------------------------------------------------ under the sanitizers
def test_the_mirror_as_a_program_under_asan_ubsan(tmp_path):
    exe = tmp_path / "featlin_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "featlin_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " cases, 0 failures" in r.stdout


def test_altered_buffers_are_clamped_and_truncated_ones_refused(mirror):
    x = fm.random_sparse(40, 300, 290, np.float32, seed=2)
    p = fm.plan(mirror, x)
    w = np.ones((300, 2), dtype=np.float32)
    one = fm.plan(mirror, x, "forward")                                                       # (its records are the buffer's tail)
    with pytest.raises(fm.Refused):
        fm.apply(mirror, one, w, buffer=one["buffer"][:-512])
    with pytest.raises(fm.Refused):
        fm.apply(mirror, one, np.ones((1, 40, 2), dtype=np.float32), transpose=True)          # a direction the plan lacks
    bad = p["buffer"].copy()
    d = p["desc"]
    bad[d["off_forward"]:d["off_forward"] + 8 * 41].view(np.int64)[::2] = 2 ** 50
    bad[d["rec_forward"]:d["rec_forward"] + 16 * d["nnz"]].view(np.int32)[2::4] = -9
    assert fm.apply(mirror, p, w, buffer=bad).shape == (1, 40, 2)


# ------------------------------------------------------------------------------------------------ the entry points
SIGS = {
    "rlap_feature_count": "h x N Fin flags nnz",
    "rlap_feature_plan_bytes": "N Fin nnz flags bytes",
    "rlap_feature_plan_build": "h x N Fin nnz flags plan plan_bytes desc info",
    "rlap_feature_plan_apply": "h plan desc flags w keep K Fout out info",
    "rlap_snapshot_plan_propagate": "h plan desc flags x F y info",
}
NNZ, BOUND, ARENA = 7, 4096, 555


class FeatureStub(StubLib):
    def __init__(self):
        super().__init__(SIGS)
        from rlap_amd import _lib
        self._lib = _lib

    def export(self, name, a):
        if name == "rlap_feature_count":
            self.calls.append((name, {k: a[k] for k in ("N", "Fin", "flags")}))
            a["nnz"]._obj.value = NNZ
            return self.status
        if name == "rlap_feature_plan_bytes":
            self.calls.append((name, {k: a[k] for k in ("N", "Fin", "nnz", "flags")}))
            a["bytes"]._obj.value = BOUND
            return 0
        if name == "rlap_feature_plan_build":
            self.calls.append((name, {k: a[k] for k in ("N", "Fin", "nnz", "flags", "plan_bytes")}))
            d, info = a["desc"]._obj, a["info"]._obj
            d.num_nodes, d.in_features, d.nnz, d.flags, d.magic, d.plan_bytes = a["N"], a["Fin"], a["nnz"], a["flags"], self._lib.FEAT_MAGIC, BOUND
            info.nnz, info.longest_forward, info.arena_bytes, info.host_syncs = a["nnz"], 3, ARENA, 1
            return 0
        if name == "rlap_feature_plan_apply":
            self.calls.append((name, {k: a[k] for k in ("flags", "K", "Fout")} | {"keep": a["keep"] is not None}))
            return self.status
        self.calls.append((name, {"flags": a.get("flags"), "F": a.get("F")}))
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, FeatureStub())


X = torch.tensor([[0.0, 1.0, 0.0], [2.0, 0.0, 3.0]])
DIRS = {"forward": 256, "transposed": 512, "both": 768}


@pytest.mark.parametrize("directions", ["forward", "transposed", "both"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_feature_plan_arguments(lib, dtype, directions):
    from rlap_amd import ops
    fp = ops.feature_plan(X.to(dtype), directions)
    f32 = 1 if dtype == torch.float32 else 0
    (cn, c), (qn, q), (bn, b) = lib.exports()
    assert cn == "rlap_feature_count" and c == {"N": 2, "Fin": 3, "flags": f32}
    assert qn == "rlap_feature_plan_bytes" and q == {"N": 2, "Fin": 3, "nnz": NNZ, "flags": f32 | DIRS[directions]}
    assert bn == "rlap_feature_plan_build" and b == {"N": 2, "Fin": 3, "nnz": NNZ, "flags": f32 | DIRS[directions], "plan_bytes": BOUND}
    assert isinstance(fp, ops.FeaturePlan) and (fp.num_nodes, fp.in_features, fp.nnz, fp.directions, fp.nbytes) == (2, 3, NNZ, directions, BOUND)
    assert fp.buffer.dtype == torch.uint8 and fp.info["longest_forward"] == 3 and fp.info["host_syncs"] == 1
    assert ops.last_stats["arena_bytes"] == ARENA
    assert ops.feature_plan(X).directions == "both"


def test_linear_arguments(lib):
    from rlap_amd import ops
    fp = ops.feature_plan(X)
    w = torch.ones(3, 5)
    y = fp.linear(w)
    assert y.shape == (2, 5) and lib.exports()[-1] == ("rlap_feature_plan_apply", {"flags": 32, "K": 1, "Fout": 5, "keep": False})
    y = fp.linear(w.double(), torch.ones(4, 3, dtype=torch.bool))
    assert y.shape == (4, 2, 5) and y.dtype == torch.float64
    assert lib.exports()[-1] == ("rlap_feature_plan_apply", {"flags": 0, "K": 4, "Fout": 5, "keep": True})
    assert fp.linear(w, torch.ones(1, 3, dtype=torch.uint8)).shape == (1, 2, 5)
    # the backward pass is the transposed call, on the upstream gradient, with the forward call's masks
    wg = torch.ones(3, 5, requires_grad=True)
    y = fp.linear(wg, torch.ones(2, 3, dtype=torch.bool))
    n = len(lib.exports())
    y.sum().backward()
    assert lib.exports()[n:] == [("rlap_feature_plan_apply", {"flags": 16 | 32, "K": 2, "Fout": 5, "keep": True})] and wg.grad.shape == (3, 5)
    wg.grad = None
    fp.linear(wg).sum().backward()
    assert lib.exports()[-1] == ("rlap_feature_plan_apply", {"flags": 16 | 32, "K": 1, "Fout": 5, "keep": False})
    with torch.no_grad():
        n = len(lib.exports())
        assert not fp.linear(wg).requires_grad and len(lib.exports()) == n + 1
    # a plan of one direction
    fwd = ops.feature_plan(X, "forward")
    y = fwd.linear(wg)
    with pytest.raises(RuntimeError, match="transposed"):
        y.sum().backward()
    with pytest.raises(ValueError, match="transposed lists only"):
        ops.feature_plan(X, "transposed").linear(w)


def test_host_checks_launch_nothing(lib):
    from rlap_amd import ops
    for x, kw, msg in [(X[0], {}, "x: a dense"), (X.long(), {}, "float32 or float64"), (X.half(), {}, "float32 or float64"),
                       (torch.zeros(0, 3), {}, "x: a dense"), (torch.zeros(3, 0), {}, "x: a dense"), (X.to_sparse(), {}, "dense"),
                       (X.clone().requires_grad_(), {}, "gradient"), (X, dict(directions="up"), "directions"), ([[1.0]], {}, "x: a dense")]:
        with pytest.raises(ValueError, match=msg):
            ops.feature_plan(x, **kw)
    assert lib.exports() == [] and ops.last_stats is None
    fp = ops.feature_plan(X)
    n = len(lib.exports())
    w = torch.ones(3, 5)
    for args, msg in [((torch.ones(4, 5),), "weight"), ((torch.ones(3),), "weight"), ((torch.ones(3, 0),), "weight"), ((w.half(),), "weight"),
                      ((w.long(),), "weight"), ((w, torch.ones(2, 4, dtype=torch.bool)), "keep"), ((w, torch.ones(3, dtype=torch.bool)), "keep"),
                      ((w, torch.ones(2, 3)), "keep"), ((w, torch.ones(0, 3, dtype=torch.bool)), "views"),
                      ((w, torch.ones(33, 3, dtype=torch.bool)), "views"), ((w.to("meta"),), "device")]:
        with pytest.raises(ValueError, match=msg):
            fp.linear(*args)
    for args, msg in [((0, 0.3), "in_features"), ((3, 1.5), "p:"), ((3, True), "p:"), ((3, 0.3, 0), "views"), ((3, 0.3, 33), "views"), ((2.5, 0.3), "in_features")]:
        with pytest.raises(ValueError, match=msg):
            ops.feature_masks(*args)
    assert len(lib.exports()) == n


@pytest.mark.parametrize("status,error", [(3, ValueError), (9, RuntimeError), (10, RuntimeError)])
def test_device_statuses(lib, status, error):
    from rlap_amd import ops
    fp = ops.feature_plan(X)
    lib.status = status
    with pytest.raises(error, match=f"status {status}"):
        fp.linear(torch.ones(3, 2))
    with pytest.raises(error, match=f"status {status}"):
        ops.feature_plan(X)


class _Snaps:
    def __init__(self):
        self.seen = None

    def propagate(self, x, transpose=False):
        self.seen = x
        return x if x.dim() == 3 else x.unsqueeze(0)


def test_gcn_conv_takes_a_feature_plan(lib):
    from rlap_amd import adapters, ops
    conv = adapters.SnapshotGCNConv(3, 5)
    fp, snaps = ops.feature_plan(X), _Snaps()
    keep = torch.ones(2, 3, dtype=torch.bool)
    out = conv(fp, snaps, keep=keep)
    assert out.shape == (2, 2, 5) and snaps.seen.shape == (2, 2, 5)
    assert lib.exports()[-1] == ("rlap_feature_plan_apply", {"flags": 32, "K": 2, "Fout": 5, "keep": True})
    assert conv(fp, snaps).shape == (1, 2, 5) and snaps.seen.shape == (2, 5)                  # no masks: x @ W, shared by the layers
    n = len(lib.exports())
    assert torch.equal(conv(X, snaps), (X @ conv.weight + conv.bias).unsqueeze(0)) and len(lib.exports()) == n   # a tensor x: as before
    with pytest.raises(ValueError, match="keep goes with"):
        conv(X, snaps, keep=keep)
    assert "feature_plan" in adapters.drop_feature.__doc__


# ------------------------------------------------------------------------------------------------ the real library, host side
BAD_ARG, TOO_LARGE = 3, 9


def test_size_query_on_the_real_library(mirror):
    from rlap_amd import _lib
    lib = _lib.load()
    b = ctypes.c_size_t(0)
    for (N, Fin, nnz), directions in [((520, 520, 2600), "both"), ((1, 1, 0), "both"), ((34493, 8415, 1103776), "forward"), ((7, 300, 257), "transposed")]:
        for f32 in (0, 1):
            assert lib.rlap_feature_plan_bytes(N, Fin, nnz, f32 | DIRS[directions], ctypes.byref(b)) == 0
            assert b.value == fm.layout(mirror, N, Fin, nnz, directions)["bytes"]
    assert lib.rlap_feature_plan_bytes(5, 6, 7, 0, ctypes.byref(b)) == 0 and b.value == fm.layout(mirror, 5, 6, 7, "both")["bytes"]   # neither flag: both
    for args, status in [((0, 5, 1, 768), BAD_ARG), ((5, 0, 1, 768), BAD_ARG), ((5, 5, -1, 768), BAD_ARG), ((-1, 5, 1, 768), BAD_ARG),
                         ((5, 5, 1, 2), BAD_ARG), ((5, 5, 1, 16), BAD_ARG), ((2 ** 31, 5, 1, 768), TOO_LARGE), ((5, 2 ** 31, 1, 768), TOO_LARGE),
                         ((5, 5, 2 ** 31 - 1, 768), TOO_LARGE), ((2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 2, 768), 0)]:
        assert lib.rlap_feature_plan_bytes(*args, ctypes.byref(b)) == status, args
    assert lib.rlap_feature_plan_bytes(5, 5, 1, 768, None) == BAD_ARG
    assert mirror.featlin_magic() == _lib.FEAT_MAGIC and mirror.featlin_max_views() == _lib.FEAT_MAX_VIEWS and mirror.featlin_chunk() == CHUNK


def test_exports_are_declared_and_listed():
    from rlap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rlap_feature_count", "rlap_feature_plan_bytes", "rlap_feature_plan_build", "rlap_feature_plan_apply"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"RLAP_FEAT_X_F32 = %d\b" % _lib.FEAT_X_F32, hdr)


@pytest.mark.parametrize("c_name,py_name", [("rlap_feature_desc", "FeatureDesc"), ("rlap_feature_info", "FeatureInfo")])
def test_layout_matches_the_header(tmp_path, c_name, py_name):
    """tests/test_cabi_symbols.py's method: a C99 program compiled against the header prints sizeof and every offsetof, compared with
    what ctypes computes for the Python structure."""
    import shutil
    from rlap_amd import _lib
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the C layout"
    cls = getattr(_lib, py_name)
    fields = [f for f, _ in cls._fields_]
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    end = hdr.index("} %s;" % c_name)
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S)
    declared = [name for decl in re.findall(r"\b(?:int32_t|int64_t|float|double)\s+([a-z_0-9, ]+);", body) for name in decl.split(", ")]
    assert declared == fields, f"the header's fields and _lib.{py_name} differ in name or order"
    src = tmp_path / "layout.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rlap_hip.h"', "int main(void) {", f'    printf("sizeof %zu\\n", sizeof({c_name}));']
    lines += [f'    printf("{f} %zu\\n", offsetof({c_name}, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(cls)
    assert {f: int(v) for f, v in got.items()} == {f: getattr(cls, f).offset for f in fields}
    assert ctypes.sizeof(cls) % 8 == 0


# ------------------------------------------------------------------------------------------------ the masks
@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("views", [1, 2, 5])
def test_feature_masks_against_drop_feature(p, views):
    from rlap_amd import adapters, ops
    x = torch.rand(9, 41) + 0.5
    g1, g2 = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
    keep = ops.feature_masks(41, p, views, generator=g1)
    dropped = adapters.drop_feature(x, p, views, generator=g2)
    assert keep.shape == (views, 41) and keep.dtype == torch.bool
    for k in range(views):
        assert torch.equal(x * keep[k], dropped[k])
    assert bool(keep.all()) if p == 0.0 else True
    assert not bool(keep.any()) if p == 1.0 else True
    assert torch.equal(g1.get_state(), g2.get_state())                                        # the same draws, no more
