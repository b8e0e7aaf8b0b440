"""GCN propagation without a GPU: the summation order of rlap_amd/csrc/rlap_spmm.h (compiled here with g++, the same source
rlap_spmm.hip includes) bit for bit against a numpy restatement of the rule, the host-side argument checks of
ops.snapshot_propagate, the adapters' new classes, and the export."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import spmm_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return spmm_mirror.build(tmp_path_factory.mktemp("spmm"))


def header_chunk():
    """C as the header states it (read, not copied)."""
    text = open(spmm_mirror.HDR).read()
    return int(re.search(r"constexpr\s+int\s+CHUNK\s*=\s*(\d+)\s*;", text).group(1))


def bits(v):
    return np.float64(v).view(np.int64)


def numpy_rule(c, x, C, loop=None):
    """The order rule restated: chunks of C entries, each summed from 0 in list order (the product rounded, then the add); the
    chunk sums added to 0 in chunk order; the loop term last.  numpy float64 scalars round every operation."""
    c, x = np.asarray(c, dtype=np.float64), np.asarray(x, dtype=np.float64)
    total = np.float64(0.0)
    for k0 in range(0, c.size, C):
        s = np.float64(0.0)
        for e in range(k0, min(k0 + C, c.size)):
            s = s + c[e] * x[e]
        total = total + s
    if loop is not None:
        total = total + np.float64(loop[0]) * np.float64(loop[1])
    return total


def test_chunk_is_the_headers(mirror):
    C = header_chunk()
    assert mirror.spmm_chunk() == C and C >= 64


def lengths(C):
    return [0, 1, 2, C - 1, C, C + 1, 2 * C, 2 * C + 1, 2 * C + 37, 5 * C + 3]


@pytest.mark.parametrize("with_loop", [False, True])
def test_lists_against_the_numpy_rule(mirror, with_loop):
    C = header_chunk()
    rs = np.random.RandomState(3)
    for n in lengths(C):
        for trial in range(3):
            c = rs.rand(n) * 10.0 ** rs.randint(-3, 4, n)
            x = rs.randn(n) * 10.0 ** rs.randint(-3, 4, n)
            loop = (rs.rand() + 0.1, rs.randn()) if with_loop else None
            got, ref = spmm_mirror.list_sum(mirror, c, x, loop), numpy_rule(c, x, C, loop)
            assert bits(got) == bits(ref), (n, trial, got, ref)
    assert bits(spmm_mirror.list_sum(mirror, [], [])) == bits(0.0)                       # an id without entries and without a loop
    assert spmm_mirror.list_sum(mirror, [], [], (0.5, 3.0)) == 1.5
    assert spmm_mirror.list_sum(mirror, [2.0], [0.25]) == 0.5


def test_the_order_is_pinned_not_incidental(mirror):
    """For long lists the rule's result differs from numpy's pairwise np.sum and from one running sum over the whole list."""
    C = header_chunk()
    rs = np.random.RandomState(4)
    differs_sum, differs_running = 0, 0
    for n in (C + 1, 2 * C + 37, 5 * C + 3):
        for trial in range(8):
            c, x = rs.rand(n), rs.randn(n)
            got = spmm_mirror.list_sum(mirror, c, x)
            differs_sum += int(bits(got) != bits(np.sum(c * x)))
            differs_running += int(bits(got) != bits(numpy_rule(c, x, 10 ** 9)))
            assert abs(got - np.sum(c * x)) <= 4 * n * 2.0 ** -53 * np.sum(np.abs(c * x))
    assert differs_sum >= 1 and differs_running >= 1


def test_entry_lists_forward_and_transposed(mirror):
    """spmm_entries groups by target (forward) or source (transposed) in list order, the loop last."""
    C = header_chunk()
    rs = np.random.RandomState(5)
    N, F, n_hub = 40, 3, 2 * C + 9
    src = np.concatenate([rs.randint(1, N, n_hub), np.arange(N), rs.randint(0, N, 50)])
    dst = np.concatenate([np.zeros(n_hub, dtype=np.int64), np.arange(N), rs.randint(0, N, 50)])
    keep = (src != dst) | (np.arange(src.size) >= n_hub) & (np.arange(src.size) < n_hub + N)   # loops only from the arange part
    src, dst = src[keep], dst[keep]
    val, x = rs.rand(src.size), rs.randn(N, F)
    for transpose in (False, True):
        y = spmm_mirror.entries(mirror, src, dst, val, N, x, True, transpose)
        key, other = (src, dst) if transpose else (dst, src)
        for j in range(N):
            sel = np.flatnonzero((key == j) & (src != dst))
            lp = np.flatnonzero((src == j) & (dst == j))
            for f in range(F):
                ref = numpy_rule(val[sel], x[other[sel], f], C, (val[lp[-1]], x[j, f]) if lp.size else None)
                assert bits(y[j, f]) == bits(ref), (transpose, j, f)
    y = spmm_mirror.entries(mirror, src, dst, val, N, x, False, False)                   # loops kept as entries like the others
    sel = np.flatnonzero(dst == 0)
    assert bits(y[0, 1]) == bits(numpy_rule(val[sel], x[src[sel], 1], C))


# ------------------------------------------------------------------------------------------------ arguments, without a device
SC = torch.tensor([[1, 0, 1.0], [0, 1, 1.0], [2, 1, 1.0], [1, 2, 1.0]], dtype=torch.float64)


@pytest.mark.parametrize("kw, match", [
    (dict(x=torch.zeros(3)), "x:"),                                              # rank
    (dict(x=torch.zeros(1, 1, 3, 2)), "x:"),
    (dict(x=torch.zeros(4, 2)), "rows"),                                         # row count
    (dict(x=torch.zeros(2, 4, 2)), "rows"),
    (dict(x=torch.zeros(3, 3, 2)), "layers"),                                    # L
    (dict(x=torch.zeros(1, 3, 2), ptr=[0, 2, 4]), "layers"),
    (dict(x=torch.zeros(3, 2, dtype=torch.float16)), "float"),                   # dtype
    (dict(x=torch.zeros(3, 2, dtype=torch.int64)), "float"),
    (dict(x=torch.zeros(3, 0)), "feature"),                                      # F == 0
    (dict(x=np.zeros((3, 2))), "x:"),
    (dict(ptr=[0, 3]), "ptr"),
    (dict(ptr=[1, 4]), "ptr"),
    (dict(ptr=[0, 3, 2, 4]), "ptr"),
    (dict(node_ptr=[0, 2]), "node_ptr"),
    (dict(node_ptr=[0, 1, 3], ptr=[0, 4]), "graphs"),
    (dict(fill_value=0.0), "fill_value"),
    (dict(fill_value=float("inf")), "fill_value"),
    (dict(fill_value="1"), "fill_value"),
    (dict(num_nodes=-1), "num_nodes"),
    (dict(sc=torch.zeros(4, 2)), "sc"),
])
def test_argument_errors_need_no_device(kw, match):
    from rlap_amd import ops
    args = dict(sc=SC, ptr=[0, 4], num_nodes=3, x=torch.zeros(3, 2))
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        ops.snapshot_propagate(args.pop("sc"), args.pop("ptr"), args.pop("num_nodes"), args.pop("x"), **args)


def test_signature_and_adapters():
    from rlap_amd import adapters, ops
    sig = inspect.signature(ops.snapshot_propagate)
    assert list(sig.parameters) == ["sc", "ptr", "num_nodes", "x", "node_ptr", "weighted", "add_self_loops", "fill_value", "normalize",
                                    "transpose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["node_ptr"], d["weighted"], d["add_self_loops"], d["fill_value"], d["normalize"], d["transpose"]) == (None, False, True, 1.0, True, False)
    for cls in (adapters.rLap, adapters.rLapViews, adapters.rLapDepths):
        assert callable(getattr(cls, "snapshots"))
    snaps = adapters.Snapshots(SC, [0, 2, 4], 3, weighted=True, fill_value=2.0)
    assert snaps.layers == 2 and snaps.weighted and snaps.fill_value == 2.0 and snaps.num_nodes == 3
    assert adapters.Snapshots(SC, [0, 1, 2, 3, 4], 3, node_ptr=[0, 1, 3]).layers == 2
    with pytest.raises(ValueError, match="rows"):
        snaps.propagate(torch.zeros(5, 2))
    torch.manual_seed(0)
    conv = adapters.SnapshotGCNConv(8, 5)
    assert isinstance(conv, torch.nn.Module) and conv.weight.shape == (8, 5) and conv.bias.shape == (5,)
    assert bool((conv.bias == 0).all())                                          # zeros, and Glorot: uniform within sqrt(6 / (in + out))
    a = (6.0 / 13.0) ** 0.5
    assert float(conv.weight.detach().abs().max()) <= a and float(conv.weight.detach().std()) > 0.3 * a
    assert adapters.SnapshotGCNConv(8, 5, bias=False).bias is None
    assert [n for n, _ in conv.named_parameters()] == ["weight", "bias"]


def test_export_is_declared():
    from rlap_amd import _lib
    assert "rlap_snapshot_propagate" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    for name in ("rlap_snapshot_propagate", "RLAP_SPMM_TRANSPOSE", "RLAP_SPMM_X_F32", "RLAP_SPMM_X_PER_LAYER", "rlap_spmm_info"):
        assert name in hdr
    m = re.search(r"enum \{ RLAP_SPMM_TRANSPOSE = (\d+), RLAP_SPMM_X_F32 = (\d+), RLAP_SPMM_X_PER_LAYER = (\d+) \}", hdr)
    assert tuple(int(v) for v in m.groups()) == (_lib.SPMM_TRANSPOSE, _lib.SPMM_X_F32, _lib.SPMM_X_PER_LAYER)
    assert ctypes_size(_lib.SpmmInfo) == 4 * 8 + 2 * 4


def ctypes_size(cls):
    import ctypes
    return ctypes.sizeof(cls)
