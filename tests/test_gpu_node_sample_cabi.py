"""rlap_node_sample called through the C ABI on a handle of the test's own (the arena the library owns): the result against the host
mirror, the optional outputs left out, and every refusal -- the host's and the device's -- with the right status and, for too small an
out_cap_rows, the needed rows in the info struct, which is zeroed first."""
import ctypes

import numpy as np
import pytest
import torch

import node_sample_cases as cases
import nodesample_mirror

pytestmark = pytest.mark.gpu

OK, INDEX_RANGE, BAD_ARG, TOO_LARGE, OUT_CAPACITY = 0, 2, 3, 9, 13
DROP, WALK = 0, 1
L = 5


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib
    src, dst, n = cases.graph("two_ba50")
    mirror = nodesample_mirror.build(tmp_path_factory.mktemp("nodesample"))
    return {"lib": _lib.load(), "_lib": _lib, "src": src, "dst": dst, "n": n, "d_src": torch.from_numpy(src).cuda(),
            "d_dst": torch.from_numpy(dst).cuda(), "d_w": torch.from_numpy(cases.weights(src.size)).cuda(), "mirror": mirror}


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def call(env, h, scheme=DROP, p=(0.3, 0.45), seeds=(40, 25), K=None, walk_length=L, seed=cases.SEED, cap=None, n=None, src=None, dst=None,
         weighted=True, outputs=True, ptr=True, params=True, walks=None):
    """One rlap_node_sample on the handle; the info struct holds 0xFF bytes before the call.  Returns (status, info, buffers)."""
    _lib = env["_lib"]
    E = env["src"].size
    values = seeds if scheme == WALK else p
    K = len(values) if K is None else K
    cap = K * E if cap is None else cap
    dev = env["d_src"].device
    walkers = sum(s for s in seeds if 0 <= s < 2**20) if scheme == WALK else 0
    bufs = {"rows": torch.full((max(cap, 1), 3), -7.0, dtype=torch.float64, device=dev), "ptr": torch.full((K + 1,), -7, dtype=torch.int64, device=dev),
            "nodes": torch.full((max(K, 1), env["n"]), 7, dtype=torch.uint8, device=dev),
            "walks": torch.full((max(walkers, 1), max(walk_length, 0) % 2048 + 1), -7, dtype=torch.int64, device=dev)}
    info = _lib.NodeSampleInfo()
    ctypes.memset(ctypes.addressof(info), 0xFF, ctypes.sizeof(info))
    hp = (ctypes.c_double * max(len(p), 1))(*p)
    hs = (ctypes.c_int64 * max(len(seeds), 1))(*seeds)
    want_walks = (scheme == WALK and outputs) if walks is None else walks
    torch.cuda.synchronize()
    rc = env["lib"].rlap_node_sample(h, (env["d_src"] if src is None else src).data_ptr(), (env["d_dst"] if dst is None else dst).data_ptr(),
                                     env["d_w"].data_ptr() if weighted else None, E, env["n"] if n is None else n, scheme,
                                     hp if params and scheme == DROP else None, hs if params and scheme == WALK else None, K, walk_length, seed,
                                     bufs["rows"].data_ptr() if cap else None, cap, bufs["ptr"].data_ptr() if ptr else None,
                                     bufs["nodes"].data_ptr() if outputs else None, bufs["walks"].data_ptr() if want_walks else None,
                                     ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, info, bufs


@pytest.mark.parametrize("scheme,name", [(DROP, "drop"), (WALK, "walk")])
def test_result_equals_the_mirror(env, handle, scheme, name):
    want = nodesample_mirror.run(env["mirror"], env["src"], env["dst"], env["n"], w=env["d_w"].cpu().numpy(), scheme=name, p=(0.3, 0.45),
                                 num_seeds=(40, 25), walk_length=L, seed=cases.SEED)
    rc, info, b = call(env, handle, scheme=scheme)
    total = int(want["ptr"][-1])
    assert rc == OK and info.rows_needed == total and info.host_syncs == 1 and info.arena_bytes > 0 and info.launches > 0 and info.pad == 0
    assert total > 0 and b["ptr"].tolist() == want["ptr"].tolist() and np.array_equal(b["rows"][:total].cpu().numpy(), want["rows"])
    assert bool((b["rows"][total:] == -7.0).all())                                  # nothing behind the last row
    assert np.array_equal(b["nodes"].cpu().numpy().astype(bool), want["nodes"]) and int(b["nodes"].max()) <= 1
    if scheme == WALK:
        assert np.array_equal(b["walks"].cpu().numpy(), want["walks"])
    rc, info2, b2 = call(env, handle, scheme=scheme, outputs=False, weighted=False)
    assert rc == OK and info2.rows_needed == total and torch.equal(b2["rows"][:total, :2], b["rows"][:total, :2])
    assert bool((b2["rows"][:total, 2] == 1.0).all()) and bool((b2["nodes"] == 7).all()) and bool((b2["walks"] == -7).all())
    assert info2.launches < info.launches                                           # the node mask has kernels of its own


def test_refusals(env, handle):
    E, n = env["src"].size, env["n"]
    for scheme in (DROP, WALK):
        full = call(env, handle, scheme=scheme)[1].rows_needed
        assert 0 < full < 2 * E
        # too little room: nothing written, the needed rows reported
        rc, info, b = call(env, handle, scheme=scheme, cap=full - 1)
        assert rc == OUT_CAPACITY and info.rows_needed == full and info.host_syncs == 1 and bool((b["rows"] == -7.0).all())
        rc, info, b = call(env, handle, scheme=scheme, cap=0)
        assert rc == OUT_CAPACITY and info.rows_needed == full
        rc, info, b = call(env, handle, scheme=scheme, cap=full)
        assert rc == OK and info.rows_needed == full and bool((b["rows"][:full, 2] > 0).all())
        # an id out of range is found on the device
        for col, row, value in ((0, 5, n), (1, 9, -1), (1, E - 1, 2**40)):
            bad = [env["d_src"].clone(), env["d_dst"].clone()]
            bad[col][row] = value
            rc, info, b = call(env, handle, scheme=scheme, src=bad[0], dst=bad[1])
            assert rc == INDEX_RANGE and info.rows_needed == 0 and info.host_syncs == 1 and bool((b["rows"] == -7.0).all())
        rc, info, _ = call(env, handle, scheme=scheme, n=n - 1)
        assert rc == INDEX_RANGE
    # host-side refusals: the info struct zeroed, nothing launched
    for kw, status in [(dict(p=(0.5,) * 33), TOO_LARGE), (dict(p=(0.3, 1.5)), BAD_ARG), (dict(p=(-0.1,)), BAD_ARG), (dict(p=(float("nan"),)), BAD_ARG),
                       (dict(p=(0.5,), K=0), BAD_ARG), (dict(scheme=2), BAD_ARG), (dict(scheme=-1), BAD_ARG), (dict(n=-1), BAD_ARG),
                       (dict(n=2**31), TOO_LARGE), (dict(ptr=False), BAD_ARG), (dict(params=False), BAD_ARG), (dict(walks=True), BAD_ARG),
                       (dict(scheme=WALK, params=False), BAD_ARG), (dict(scheme=WALK, seeds=(3, -1)), BAD_ARG),
                       (dict(scheme=WALK, seeds=(2**31,)), TOO_LARGE), (dict(scheme=WALK, seeds=(1,) * 33), TOO_LARGE),
                       (dict(scheme=WALK, walk_length=-1), BAD_ARG), (dict(scheme=WALK, walk_length=1025), BAD_ARG),
                       (dict(scheme=WALK, n=0), BAD_ARG)]:
        rc, info, b = call(env, handle, **kw)
        assert rc == status, (kw, rc)
        assert bytes(info) == bytes(ctypes.sizeof(info)), kw
        assert bool((b["rows"] == -7.0).all()) and bool((b["ptr"] == -7).all()) and bool((b["walks"] == -7).all())
    assert env["lib"].rlap_node_sample(None, *([None] * 3), 0, 0, 0, (ctypes.c_double * 1)(0.5), None, 1, 0, 0, None, 0, None, None, None, None) == BAD_ARG
    rc, info, _ = call(env, handle)                                                 # the handle works after the refusals
    assert rc == OK and info.rows_needed > 0
