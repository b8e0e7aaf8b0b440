"""rlap_edge_add called through the C ABI: on a handle of the test's own (the arena the library owns) and on a caller-owned workspace;
the result against the host mirror, the optional outputs left out, added rows without an input row (which only the C ABI can ask
for), and every refusal -- the host's and the device's -- with the right status and, for too small an out_cap_rows, the needed rows
in the info struct, which is zeroed first."""
import ctypes

import numpy as np
import pytest
import torch

import edge_add_cases as cases
import edgeadd_mirror

pytestmark = pytest.mark.gpu

OK, INDEX_RANGE, BAD_ARG, TOO_LARGE, WORKSPACE, OUT_CAPACITY = 0, 2, 3, 9, 11, 13
COALESCE = 1


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib
    src, dst, n = cases.graph("two_ba50")
    mirror = edgeadd_mirror.build(tmp_path_factory.mktemp("edgeadd"))
    return {"lib": _lib.load(), "_lib": _lib, "src": src, "dst": dst, "n": n, "d_src": torch.from_numpy(src).cuda(),
            "d_dst": torch.from_numpy(dst).cuda(), "d_w": torch.from_numpy(cases.weights(src.size)).cuda(), "mirror": mirror}


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def call(env, h, num_add=(120, 160), K=None, seed=cases.SEED, flags=COALESCE, cap=None, n=None, E=None, src=None, dst=None, weighted=True,
         outputs=True, ptr=True, counts=True, aptr=None):
    """One rlap_edge_add on the handle; the info struct holds 0xFF bytes before the call.  Returns (status, info, buffers)."""
    _lib = env["_lib"]
    E = env["src"].size if E is None else E
    K = len(num_add) if K is None else K
    total_add = sum(c for c in num_add if 0 <= c < 2**20)
    cap = K * E + total_add if cap is None else cap
    dev = env["d_src"].device
    bufs = {"rows": torch.full((max(cap, 1), 3), -7.0, dtype=torch.float64, device=dev), "ptr": torch.full((K + 1,), -7, dtype=torch.int64, device=dev),
            "added": torch.full((max(total_add, 1), 2), -7, dtype=torch.int64, device=dev), "aptr": torch.full((K + 1,), -7, dtype=torch.int64, device=dev)}
    info = _lib.EdgeAddInfo()
    ctypes.memset(ctypes.addressof(info), 0xFF, ctypes.sizeof(info))
    hc = (ctypes.c_int64 * max(len(num_add), 1))(*num_add)
    want_aptr = outputs if aptr is None else aptr
    torch.cuda.synchronize()
    rc = env["lib"].rlap_edge_add(h, (env["d_src"] if src is None else src).data_ptr(), (env["d_dst"] if dst is None else dst).data_ptr(),
                                  env["d_w"].data_ptr() if weighted else None, E, env["n"] if n is None else n, hc if counts else None, K, seed, flags,
                                  bufs["rows"].data_ptr() if cap else None, cap, bufs["ptr"].data_ptr() if ptr else None,
                                  bufs["added"].data_ptr() if outputs else None, bufs["aptr"].data_ptr() if want_aptr else None, ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, info, bufs


@pytest.mark.parametrize("flags", [COALESCE, 0])
def test_result_equals_the_mirror(env, handle, flags):
    want = edgeadd_mirror.run(env["mirror"], env["src"], env["dst"], env["n"], w=env["d_w"].cpu().numpy(), num_add=(120, 160), seed=cases.SEED,
                              coalesce=bool(flags))
    rc, info, b = call(env, handle, flags=flags)
    total = int(want["ptr"][-1])
    assert rc == OK and info.rows_needed == total and info.added == 280 and info.arena_bytes > 0 and info.launches > 0 and info.pad == 0
    assert (info.host_syncs, info.sorts, info.input_sorted, info.input_distinct) == ((1, 2, 0, want["input_distinct"]) if flags else (1, 0, 0, 0))
    assert total > 0 and b["ptr"].tolist() == want["ptr"].tolist() and np.array_equal(b["rows"][:total].cpu().numpy(), want["rows"])
    assert bool((b["rows"][total:] == -7.0).all())                                  # nothing behind the last row
    assert np.array_equal(b["added"].cpu().numpy(), want["added"]) and b["aptr"].tolist() == want["aptr"].tolist()
    rc, info2, b2 = call(env, handle, flags=flags, outputs=False, weighted=False)
    assert rc == OK and info2.rows_needed == total and torch.equal(b2["rows"][:total, :2], b["rows"][:total, :2])
    assert bool((b2["added"] == -7).all()) and bool((b2["aptr"] == -7).all())


def test_added_rows_without_an_input_row(env, handle):
    """E = 0 with rows to add: list A is empty and a view is its distinct draws, each with its count."""
    for num_add in ((1,), (cases.T - 1, cases.T, cases.T + 1), (2 * cases.T + 1, 0)):
        empty = np.zeros(0, dtype=np.int64)
        want = edgeadd_mirror.run(env["mirror"], empty, empty, 50, num_add=num_add, seed=3)
        rc, info, b = call(env, handle, num_add=num_add, E=0, n=50, seed=3, weighted=False)
        total = int(want["ptr"][-1])
        assert rc == OK and info.rows_needed == total and info.input_distinct == 0 and info.input_sorted == 1 and info.host_syncs == 1 and info.sorts == 1
        assert b["ptr"].tolist() == want["ptr"].tolist() and np.array_equal(b["rows"][:total].cpu().numpy(), want["rows"])
        assert np.array_equal(b["added"][:sum(num_add)].cpu().numpy(), want["added"])


def test_caller_owned_workspace(env, handle):
    lib = env["lib"]
    need, rn = ctypes.c_size_t(0), ctypes.c_int64(0)
    small = torch.empty(4096, dtype=torch.uint8, device="cuda")
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, small.data_ptr(), small.numel(), rng.data_ptr(), rng.numel()) == 0
    rc, info, b = call(env, handle)
    assert rc == WORKSPACE and bool((b["rows"] == -7.0).all())
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == 0 and need.value > 4096
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), ws.numel(), rng.data_ptr(), rng.numel()) == 0
    want = edgeadd_mirror.run(env["mirror"], env["src"], env["dst"], env["n"], w=env["d_w"].cpu().numpy(), num_add=(120, 160), seed=cases.SEED)
    rc, info, b = call(env, handle)
    total = int(want["ptr"][-1])
    assert rc == OK and info.rows_needed == total and 0 < info.arena_bytes <= need.value
    assert np.array_equal(b["rows"][:total].cpu().numpy(), want["rows"]) and b["ptr"].tolist() == want["ptr"].tolist()


def test_refusals(env, handle):
    E, n = env["src"].size, env["n"]
    for flags in (COALESCE, 0):
        full = call(env, handle, flags=flags)[1].rows_needed
        assert E < full <= 2 * E + 280
        # too little room: nothing written, the needed rows reported
        rc, info, b = call(env, handle, flags=flags, cap=full - 1)
        assert rc == OUT_CAPACITY and info.rows_needed == full and bool((b["rows"] == -7.0).all())
        rc, info, b = call(env, handle, flags=flags, cap=0)
        assert rc == OUT_CAPACITY and info.rows_needed == full
        rc, info, b = call(env, handle, flags=flags, cap=full)
        assert rc == OK and info.rows_needed == full and bool((b["rows"][:full, 2] > 0).all())
        # an id out of range is found on the device
        for col, row, value in ((0, 5, n), (1, 9, -1), (1, E - 1, 2**40)):
            bad = [env["d_src"].clone(), env["d_dst"].clone()]
            bad[col][row] = value
            rc, info, b = call(env, handle, flags=flags, src=bad[0], dst=bad[1])
            assert rc == INDEX_RANGE and info.rows_needed == 0 and info.host_syncs == 1 and bool((b["rows"] == -7.0).all())
        rc, info, _ = call(env, handle, flags=flags, n=n - 1)
        assert rc == INDEX_RANGE
    # host-side refusals: the info struct zeroed, nothing launched
    for kw, status in [(dict(num_add=(1,) * 33), TOO_LARGE), (dict(num_add=(3, -1)), BAD_ARG), (dict(num_add=(5,), K=0), BAD_ARG),
                       (dict(num_add=(2**31 - 1 - E,)), TOO_LARGE), (dict(n=2**31), TOO_LARGE), (dict(n=-1), BAD_ARG), (dict(flags=2), BAD_ARG),
                       (dict(ptr=False), BAD_ARG), (dict(counts=False), BAD_ARG), (dict(aptr=False), BAD_ARG), (dict(outputs=False, aptr=True), BAD_ARG),
                       (dict(E=0, n=1, num_add=(1,)), BAD_ARG), (dict(E=0, n=0, num_add=(0, 2)), BAD_ARG)]:
        rc, info, b = call(env, handle, **kw)
        assert rc == status, (kw, rc)
        assert bytes(info) == bytes(ctypes.sizeof(info)), kw
        assert bool((b["rows"] == -7.0).all()) and bool((b["ptr"] == -7).all()) and bool((b["added"] == -7).all())
    assert env["lib"].rlap_edge_add(None, None, None, None, 0, 0, (ctypes.c_int64 * 1)(0), 1, 0, 1, None, 0, None, None, None, None) == BAD_ARG
    rc, info, _ = call(env, handle)                                                 # the handle works after the refusals
    assert rc == OK and info.rows_needed > 0
