"""rlap_edge_drop called through the C ABI on a handle of the test's own (the arena the library owns): the result against the host
mirror, the optional outputs left out, and every refusal -- the host's and the device's -- with the right status and, for too small an
out_cap_rows, the needed rows in the info struct, which is zeroed first."""
import ctypes

import numpy as np
import pytest
import torch

import edge_drop_cases as cases
import edgedrop_mirror

pytestmark = pytest.mark.gpu

OK, INDEX_RANGE, BAD_ARG, TOO_LARGE, OUT_CAPACITY = 0, 2, 3, 9, 13


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib
    src, dst, n = cases.graph("two_ba50")
    mirror = edgedrop_mirror.build(tmp_path_factory.mktemp("edgedrop"))
    return {"lib": _lib.load(), "_lib": _lib, "src": src, "dst": dst, "n": n, "d_src": torch.from_numpy(src).cuda(),
            "d_dst": torch.from_numpy(dst).cuda(), "d_w": torch.from_numpy(cases.weights(src.size)).cuda(), "mirror": mirror}


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def call(env, h, scheme=1, flags=0, p=(0.3, 0.45), K=None, threshold=0.7, seed=cases.SEED, damp=0.85, pr_iters=10, evc_tol=1e-6, evc_max_iter=1000,
         cap=None, n=None, src=None, dst=None, weighted=True, outputs=True, ptr=True):
    """One rlap_edge_drop on the handle; the info struct holds 0xFF bytes before the call.  Returns (status, info, buffers)."""
    _lib = env["_lib"]
    E = env["src"].size
    K = len(p) if K is None else K
    cap = K * E if cap is None else cap
    dev = env["d_src"].device
    bufs = {"rows": torch.full((max(cap, 1), 3), -7.0, dtype=torch.float64, device=dev), "ptr": torch.full((K + 1,), -7, dtype=torch.int64, device=dev),
            "mask": torch.full((max(K, 1), E), 7, dtype=torch.uint8, device=dev), "centrality": torch.full((env["n"],), -7.0, dtype=torch.float64, device=dev),
            "node_weight": torch.full((env["n"],), -7.0, dtype=torch.float64, device=dev)}
    info = _lib.EdgeDropInfo()
    ctypes.memset(ctypes.addressof(info), 0xFF, ctypes.sizeof(info))
    hp = (ctypes.c_double * max(len(p), 1))(*p)
    torch.cuda.synchronize()
    rc = env["lib"].rlap_edge_drop(h, (env["d_src"] if src is None else src).data_ptr(), (env["d_dst"] if dst is None else dst).data_ptr(),
                                   env["d_w"].data_ptr() if weighted else None, E, env["n"] if n is None else n, scheme, flags, hp, K, threshold, seed,
                                   damp, pr_iters, evc_tol, evc_max_iter, bufs["rows"].data_ptr() if cap else None, cap,
                                   bufs["ptr"].data_ptr() if ptr else None, bufs["mask"].data_ptr() if outputs else None,
                                   bufs["centrality"].data_ptr() if outputs else None, bufs["node_weight"].data_ptr() if outputs else None,
                                   ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, info, bufs


@pytest.mark.parametrize("scheme,name", [(0, "uniform"), (1, "degree"), (2, "pagerank"), (3, "eigenvector")])
def test_result_equals_the_mirror(env, handle, scheme, name):
    for flags, aggr in ((0, "sink"), (1, "source")):
        want = edgedrop_mirror.run(env["mirror"], env["src"], env["dst"], env["n"], w=env["d_w"].cpu().numpy(), p=cases.PS, scheme=name,
                                   threshold=cases.THRESHOLD, seed=cases.SEED, aggr=aggr)
        assert (np.abs(want["u"] - want["q"]) > cases.BAND).all()
        rc, info, b = call(env, handle, scheme=scheme, flags=flags)
        total = int(want["ptr"][-1])
        assert rc == OK and info.rows_needed == total and info.host_syncs == 1 and info.arena_bytes > 0 and info.launches > 0 and info.pad == 0
        assert (info.iters, bool(info.converged)) == (want["iters"], want["converged"])
        assert b["ptr"].tolist() == want["ptr"].tolist() and np.array_equal(b["rows"][:total].cpu().numpy(), want["rows"])
        assert bool((b["rows"][total:] == -7.0).all())                              # nothing behind the last row
        assert np.array_equal(b["mask"].cpu().numpy().astype(bool), want["mask"]) and int(b["mask"].max()) <= 1
        assert np.array_equal(b["centrality"].cpu().numpy(), want["centrality"])
        rc, info2, b2 = call(env, handle, scheme=scheme, flags=flags, outputs=False, weighted=False)
        assert rc == OK and info2.rows_needed == total and torch.equal(b2["rows"][:total, :2], b["rows"][:total, :2])
        assert bool((b2["rows"][:total, 2] == 1.0).all()) and bool((b2["mask"] == 7).all()) and bool((b2["centrality"] == -7.0).all())


def test_refusals(env, handle):
    E, n = env["src"].size, env["n"]
    _, fit_info, fit = call(env, handle)
    full = fit_info.rows_needed
    assert 0 < full < 2 * E and int(fit["mask"].max()) <= 1
    # too little room: no row written, the needed rows reported; the edge mask is written all the same (the same seed, the same coins)
    rc, info, b = call(env, handle, cap=full - 1)
    assert rc == OUT_CAPACITY and info.rows_needed == full and info.host_syncs == 1 and bool((b["rows"] == -7.0).all())
    assert torch.equal(b["mask"], fit["mask"])
    rc, info, b = call(env, handle, cap=0)
    assert rc == OUT_CAPACITY and info.rows_needed == full
    rc, info, b = call(env, handle, cap=full)
    assert rc == OK and info.rows_needed == full and bool((b["rows"][:full, 2] > 0).all())
    # an id out of range is found on the device
    for col, row, value in ((0, 5, n), (1, 9, -1), (1, E - 1, 2**40)):
        bad = [env["d_src"].clone(), env["d_dst"].clone()]
        bad[col][row] = value
        for scheme in range(4):
            rc, info, _ = call(env, handle, scheme=scheme, src=bad[0], dst=bad[1])
            assert rc == INDEX_RANGE and info.rows_needed == 0 and info.host_syncs == 1
    rc, info, _ = call(env, handle, n=n - 1)
    assert rc == INDEX_RANGE
    # host-side refusals: the info struct zeroed, nothing launched
    for kw, status in [(dict(p=(0.5,) * 33), TOO_LARGE), (dict(p=(0.3, 1.5)), BAD_ARG), (dict(p=(-0.1,)), BAD_ARG), (dict(p=(float("nan"),)), BAD_ARG),
                       (dict(p=(0.5,), K=0), BAD_ARG), (dict(scheme=4), BAD_ARG), (dict(scheme=-1), BAD_ARG), (dict(flags=2), BAD_ARG),
                       (dict(threshold=1.5), BAD_ARG), (dict(n=-1), BAD_ARG), (dict(n=2**31), TOO_LARGE), (dict(ptr=False), BAD_ARG),
                       (dict(scheme=2, damp=1.5), BAD_ARG), (dict(scheme=2, pr_iters=-1), BAD_ARG), (dict(scheme=2, pr_iters=10**6), TOO_LARGE),
                       (dict(scheme=3, evc_max_iter=0), BAD_ARG), (dict(scheme=3, evc_tol=-1.0), BAD_ARG), (dict(scheme=3, evc_max_iter=10**6), TOO_LARGE)]:
        rc, info, b = call(env, handle, **kw)
        assert rc == status, (kw, rc)
        assert bytes(info) == bytes(ctypes.sizeof(info)), kw
        assert bool((b["rows"] == -7.0).all()) and bool((b["ptr"] == -7).all())
    assert env["lib"].rlap_edge_drop(None, *([None] * 3), 0, 0, 0, 0, (ctypes.c_double * 1)(0.5), 1, 0.7, 0, 0.85, 10, 1e-6, 10, None, 0, None, None, None,
                                     None, None) == BAD_ARG
    rc, info, _ = call(env, handle)                                                 # the handle works after the refusals
    assert rc == OK and info.rows_needed == full


def test_convergence_report(env, handle):
    rc, info, _ = call(env, handle, scheme=3, evc_tol=1e-12, evc_max_iter=3)
    assert rc == OK and (info.iters, info.converged) == (3, 0)
    rc, info, _ = call(env, handle, scheme=3, evc_tol=0.5, evc_max_iter=50)
    assert rc == OK and info.converged == 1 and 1 <= info.iters < 50
    rc, info, _ = call(env, handle, scheme=2, pr_iters=0)
    assert rc == OK and (info.iters, info.converged) == (0, 1)
