"""rlap_feature_count / rlap_feature_plan_build / rlap_feature_plan_apply called through the C ABI on a handle of the test's own: the
results against ops' (which the other files hold against the mirror), every refusal code the header names, the descriptor zeroed on
refusal, a build whose nnz is off by one, a plan of one direction used in the other, a caller's arena that is too small."""
import ctypes

import numpy as np
import pytest
import torch

import featlin_mirror as fm

pytestmark = pytest.mark.gpu

OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
FORWARD, TRANSPOSED, X_F32, SPMM_TRANSPOSE, SPMM_F32 = 256, 512, 1, 16, 32


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib, ops
    x = torch.from_numpy(fm.random_sparse(70, 300, 290, np.float32, seed=6)).cuda()
    fp = ops.feature_plan(x)
    assert fp.info["chunks_forward"] > 0
    rng = np.random.default_rng(1)
    w = torch.from_numpy(rng.uniform(-1, 1, size=(300, 8)).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.uniform(-1, 1, size=(2, 70, 8)).astype(np.float32)).cuda()
    keep = torch.from_numpy(fm.masks("random", 2, x.cpu().numpy())).cuda()
    y, dw = fp.linear(w, keep), ops._feature_apply(fp, g, keep, 2, True)
    torch.cuda.synchronize()
    return {"lib": _lib.load(), "_lib": _lib, "x": x, "fp": fp, "w": w, "g": g, "keep": keep, "y": y, "dw": dw}


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def zeroed(s):
    return bytes(ctypes.string_at(ctypes.addressof(s), ctypes.sizeof(s))) == bytes(ctypes.sizeof(s))


def count(env, h, x=None, N=70, Fin=300, flags=X_F32):
    n = ctypes.c_int64(-7)
    torch.cuda.synchronize()
    rc = env["lib"].rlap_feature_count(h, env["x"].data_ptr() if x is None else x, N, Fin, flags, ctypes.byref(n))
    return rc, int(n.value)


def bytes_of(env, nnz, flags):
    b = ctypes.c_size_t(0)
    assert env["lib"].rlap_feature_plan_bytes(70, 300, nnz, flags, ctypes.byref(b)) == OK
    return int(b.value)


def build(env, h, nnz, flags=X_F32 | FORWARD | TRANSPOSED, x="x", N=70, Fin=300, d_plan="buf", plan_bytes=None, desc="desc"):
    """One rlap_feature_plan_build; h_desc holds 0xFF bytes before the call.  Returns (status, desc, info, buf)."""
    _lib = env["_lib"]
    buf = torch.empty(bytes_of(env, min(max(nnz, 0), 10 ** 6), flags & (FORWARD | TRANSPOSED)) + 256, dtype=torch.uint8, device="cuda")
    d, info = _lib.FeatureDesc(), _lib.FeatureInfo()
    ctypes.memset(ctypes.addressof(d), 0xFF, ctypes.sizeof(d))
    torch.cuda.synchronize()
    rc = env["lib"].rlap_feature_plan_build(h, env["x"].data_ptr() if x == "x" else x, N, Fin, nnz, flags,
                                            buf.data_ptr() if d_plan == "buf" else d_plan, buf.numel() - 256 if plan_bytes is None else plan_bytes,
                                            ctypes.byref(d) if desc == "desc" else None, ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, d, info, buf


def apply(env, h, buf, desc, flags, operand, keep, K, Fout, out_shape, d_plan=None, w="w", out="out"):
    info = env["_lib"].FeatureInfo()
    res = torch.full(out_shape, float("nan"), dtype=operand.dtype, device="cuda")
    torch.cuda.synchronize()
    rc = env["lib"].rlap_feature_plan_apply(h, buf.data_ptr() if d_plan is None else d_plan, ctypes.byref(desc) if desc is not None else None, flags,
                                            operand.data_ptr() if w == "w" else w, keep.data_ptr() if keep is not None else None, K, Fout,
                                            res.data_ptr() if out == "out" else out, ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, res, info


def test_the_three_calls(env, handle):
    fp = env["fp"]
    rc, nnz = count(env, handle)
    assert rc == OK and nnz == fp.nnz == int((env["x"] != 0).sum())
    xd = env["x"].double().contiguous()
    assert count(env, handle, xd.data_ptr(), flags=0) == (OK, nnz)
    assert bytes_of(env, nnz, FORWARD | TRANSPOSED) == bytes_of(env, nnz, 0) == fp.nbytes > bytes_of(env, nnz, FORWARD)
    rc, desc, info, buf = build(env, handle, nnz)
    assert rc == OK and desc.magic == env["_lib"].FEAT_MAGIC and info.host_syncs == 1 and info.nnz == nnz and info.arena_bytes > 0
    assert {k: getattr(info, k) for k in fp.info if k != "arena_bytes"} == {k: v for k, v in fp.info.items() if k != "arena_bytes"}
    assert all(getattr(desc, k) == getattr(fp.desc, k) for k in fm.DESC)
    assert fm.same_parts(fm.decode(buf[:fp.nbytes].cpu().numpy(), desc), fm.decode(fp.buffer.cpu().numpy(), fp.desc))
    rc, y, info = apply(env, handle, buf, desc, SPMM_F32, env["w"], env["keep"], 2, 8, (2, 70, 8))
    assert rc == OK and info.host_syncs == 0 and torch.equal(y, env["y"])
    rc, dw, info = apply(env, handle, buf, desc, SPMM_F32 | SPMM_TRANSPOSE, env["g"], env["keep"], 2, 8, (300, 8))
    assert rc == OK and info.host_syncs == 0 and torch.equal(dw, env["dw"])
    rc, d2, _, b2 = build(env, handle, nnz, flags=X_F32)                                      # neither direction flag: both
    parts = fm.decode(buf.cpu().numpy(), desc)                                                # (the padding between the parts is not written)
    assert rc == OK and d2.flags == X_F32 | FORWARD | TRANSPOSED and fm.same_parts(fm.decode(b2.cpu().numpy(), d2), parts)
    rc, d3, _, b3 = build(env, handle, nnz, flags=0, x=xd.data_ptr())                         # the float64 matrix: the same lists
    assert rc == OK and d3.flags == FORWARD | TRANSPOSED and fm.same_parts(fm.decode(b3.cpu().numpy(), d3), parts)


def test_count_and_build_refusals(env, handle):
    lib = env["lib"]
    nnz = env["fp"].nnz
    for kw in (dict(x=0), dict(N=0), dict(Fin=0), dict(N=-3), dict(flags=2), dict(flags=X_F32 | FORWARD)):
        assert count(env, handle, **kw)[0] == BAD_ARG, kw
    assert count(env, handle, N=2 ** 31)[0] == TOO_LARGE and count(env, handle, Fin=2 ** 31)[0] == TOO_LARGE
    assert lib.rlap_feature_count(handle, env["x"].data_ptr(), 70, 300, X_F32, None) == BAD_ARG
    assert lib.rlap_feature_count(None, env["x"].data_ptr(), 70, 300, X_F32, ctypes.byref(ctypes.c_int64())) == BAD_ARG
    for off in (-1, 1):                                                                       # an nnz that is not the matrix's count
        rc, desc, _, _ = build(env, handle, nnz + off)
        assert rc == BAD_ARG and zeroed(desc), off
    for kw, status in [(dict(x=None), BAD_ARG), (dict(d_plan=None), BAD_ARG), (dict(N=0), BAD_ARG), (dict(Fin=-1), BAD_ARG),
                       (dict(flags=X_F32 | 2), BAD_ARG), (dict(flags=X_F32 | SPMM_TRANSPOSE), BAD_ARG), (dict(plan_bytes=256), BAD_ARG),
                       (dict(N=2 ** 31), TOO_LARGE), (dict(Fin=2 ** 31), TOO_LARGE)]:
        rc, desc, _, _ = build(env, handle, nnz, **kw)
        assert rc == status and zeroed(desc), kw
    rc, desc, _, buf = build(env, handle, nnz)
    assert build(env, handle, nnz, d_plan=buf.data_ptr() + 8)[0] == BAD_ARG                   # a misaligned buffer
    assert build(env, handle, -1)[0] == BAD_ARG and build(env, handle, 2 ** 31 - 1, plan_bytes=1 << 20)[0] == TOO_LARGE
    assert build(env, handle, nnz, desc=None)[0] == BAD_ARG
    assert build(env, handle, nnz, plan_bytes=env["fp"].nbytes - 1)[0] == BAD_ARG and build(env, handle, nnz, plan_bytes=env["fp"].nbytes)[0] == OK
    short = torch.empty(256, dtype=torch.uint8, device="cuda")                                # a caller's arena of 256 bytes
    assert lib.rlap_set_workspace(handle, short.data_ptr(), 256, None, 0) == 0
    rc, desc, _, _ = build(env, handle, nnz)
    assert rc == E_WORKSPACE and zeroed(desc) and count(env, handle)[0] == E_WORKSPACE
    need = ctypes.c_size_t(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(ctypes.c_int64())) == 0 and need.value > 256


def test_apply_refusals(env, handle):
    _lib, fp = env["_lib"], env["fp"]
    nnz = fp.nnz
    rc, desc, _, buf = build(env, handle, nnz)
    assert rc == OK
    w, g, keep = env["w"], env["g"], env["keep"]
    fwd = lambda **kw: apply(env, handle, buf, kw.pop("desc", desc), kw.pop("flags", SPMM_F32), w, kw.pop("keep", keep), kw.pop("K", 2),
                             kw.pop("Fout", 8), (2, 70, 8), **kw)[0]
    assert fwd() == OK
    for kw in (dict(K=0), dict(K=33), dict(K=-1), dict(keep=None), dict(Fout=0), dict(flags=SPMM_F32 | 64), dict(flags=SPMM_F32 | FORWARD),
               dict(w=None), dict(out=None), dict(desc=None), dict(d_plan=0), dict(d_plan=buf.data_ptr() + 4)):
        assert fwd(**kw) == BAD_ARG, kw
    assert fwd(Fout=65537) == TOO_LARGE
    assert apply(env, handle, buf, desc, SPMM_F32, w, None, 1, 8, (1, 70, 8))[0] == OK        # no masks: K = 1
    assert apply(env, None, buf, desc, SPMM_F32, w, keep, 2, 8, (2, 70, 8))[0] == BAD_ARG
    # a descriptor that is not a successful build's
    for field, value in (("magic", 0), ("magic", _lib.PLAN_MAGIC), ("nnz", -1), ("num_nodes", 0), ("in_features", 2 ** 31), ("off_forward", -256),
                         ("off_forward", 8), ("rec_forward", fp.nbytes), ("dir_forward", fp.nbytes + 256), ("chunks_forward", 10 ** 6),
                         ("plan_bytes", 1024), ("flags", X_F32 | TRANSPOSED)):
        bad = _lib.FeatureDesc.from_buffer_copy(desc)
        setattr(bad, field, value)
        assert fwd(desc=bad) == BAD_ARG, (field, value)
    assert fwd(desc=_lib.FeatureDesc()) == BAD_ARG                                            # the zeroed descriptor of a refused build
    # a plan of one direction used in the other
    for flags, has_t in ((X_F32 | FORWARD, False), (X_F32 | TRANSPOSED, True)):
        rc, d1, info, b1 = build(env, handle, nnz, flags=flags)
        assert rc == OK and (info.longest_forward == -1) == has_t and (info.longest_transposed == -1) != has_t
        rf = apply(env, handle, b1, d1, SPMM_F32, w, keep, 2, 8, (2, 70, 8))
        rt = apply(env, handle, b1, d1, SPMM_F32 | SPMM_TRANSPOSE, g, keep, 2, 8, (300, 8))
        assert (rf[0], rt[0]) == ((BAD_ARG, OK) if has_t else (OK, BAD_ARG))
        assert torch.equal(rt[1], env["dw"]) if has_t else torch.equal(rf[1], env["y"])
        refused = rf[1] if has_t else rt[1]
        assert bool(torch.isnan(refused).all())                                               # refused before any launch: nothing written
