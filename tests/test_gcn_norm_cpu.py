"""Encoder-ready snapshots without a GPU: the scalar arithmetic of rlap_amd/csrc/rlap_gcnmath.h (compiled here with g++, the same
source rlap_gcn.hip includes) against numpy, the host-side argument checks of ops.snapshot_gcn_norm, the adapters' keyword, and
the export."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_gcnmath.h")

WRAP = r"""
#include "rlap_gcnmath.h"
extern "C" {
double gm_dis(double deg) { return rlap::gcnmath::dis(deg); }
double gm_value(double di, double w, double dj) { return rlap::gcnmath::value(di, w, dj); }
float gm_round32(double v) { return rlap::gcnmath::round32(v); }
int gm_weight_ok(double w) { return rlap::gcnmath::weight_ok(w) ? 1 : 0; }
}
"""


@pytest.fixture(scope="module")
def gm(tmp_path_factory):
    d = tmp_path_factory.mktemp("gcnmath")
    src, so = d / "gm.cc", d / "libgm.so"
    src.write_text(WRAP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.dirname(HDR),
                           "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    dbl = ctypes.c_double
    lib.gm_dis.restype = dbl
    lib.gm_dis.argtypes = [dbl]
    lib.gm_value.restype = dbl
    lib.gm_value.argtypes = [dbl, dbl, dbl]
    lib.gm_round32.restype = ctypes.c_float
    lib.gm_round32.argtypes = [dbl]
    lib.gm_weight_ok.restype = ctypes.c_int
    lib.gm_weight_ok.argtypes = [dbl]
    return lib


def bits64(x):
    return np.float64(x).view(np.int64)


def test_dis_against_numpy(gm):
    assert gm.gm_dis(0.0) == 0.0 and bits64(gm.gm_dis(0.0)) == 0          # PyG's masked_fill of the infinity: +0
    for deg in (1.0, 2.0, 3.0, 1e-300, 1e300, 2.0 ** 53, 0.1, 7.0, 6190.0):
        ref = np.float64(1.0) / np.sqrt(np.float64(deg))
        assert bits64(gm.gm_dis(deg)) == bits64(ref), deg
    assert gm.gm_dis(1.0) == 1.0 and gm.gm_dis(4.0) == 0.5
    assert gm.gm_dis(-1.0) == 0.0 and gm.gm_dis(float("nan")) == 0.0      # never a NaN or an infinity out of a degree
    rs = np.random.RandomState(0)
    for deg in np.concatenate([rs.rand(200) * 100, np.arange(1, 60, dtype=np.float64)]):
        assert bits64(gm.gm_dis(float(deg))) == bits64(np.float64(1.0) / np.sqrt(np.float64(deg)))


def test_entry_values_against_numpy(gm):
    rs = np.random.RandomState(1)
    di, w, dj = rs.rand(500), rs.rand(500) * 10, rs.rand(500)
    ref = (di * w) * dj                                                      # evaluated from the left, as dis[src] * w * dis[dst]
    for k in range(500):
        assert bits64(gm.gm_value(di[k], w[k], dj[k])) == bits64(ref[k])
    # an id without rows: its loop has degree fill and value dis * fill * dis -- exactly 1 for fill = 1, within 2 roundings for 2
    d1 = gm.gm_dis(1.0)
    assert gm.gm_value(d1, 1.0, d1) == 1.0
    d2 = gm.gm_dis(2.0)
    assert abs(gm.gm_value(d2, 2.0, d2) - 1.0) <= 4 * 2.0 ** -53
    assert gm.gm_value(0.0, 5.0, 0.7) == 0.0                                 # a zero degree silences the entry


def test_float32_rounding_is_numpys(gm):
    rs = np.random.RandomState(2)
    vals = np.concatenate([rs.rand(300), rs.rand(100) * 1e-40, rs.rand(50) * 1e39, [0.0, 1.0, 1e40, -1e40, 1e-50],
                           # halfway between two float32 neighbours: ties to even
                           [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 2.0 ** -24 - 2.0 ** -53]])
    with np.errstate(over="ignore"):
        ref = vals.astype(np.float32)
    for v, r in zip(vals, ref):
        got = np.float32(gm.gm_round32(float(v)))
        assert got.view(np.int32) == r.view(np.int32), v


def test_weight_rule(gm):
    for w in (1.0, 1e-300, 1e300, 5e-324):
        assert gm.gm_weight_ok(w) == 1
    for w in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert gm.gm_weight_ok(w) == 0


# ---------------------------------------------------------------- host-side argument checks (nothing is launched: no GPU here)
SC = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]], dtype=torch.float64)


@pytest.mark.parametrize("args,kw", [
    ((SC, [0, 3], 2), {}),                               # ptr[-1] != rows
    ((SC, [1, 2], 2), {}),                               # ptr[0] != 0
    ((SC, [0, 2, 1, 2], 2), {}),                         # decreasing
    ((SC, [0], 2), {}),                                  # no segment
    ((SC, [0, 2], -1), {}),                              # num_nodes
    ((SC[:, :2], [0, 2], 2), {}),                        # not (m, 3)
    ((SC, [0, 1, 2], 2), {"node_ptr": [0, 1, 2, 2]}),   # 3 graphs do not divide 2 segments
    ((SC, [0, 2], 2), {"node_ptr": [0, 1]}),            # node_ptr[-1] != num_nodes
    ((SC, [0, 2], 2), {"node_ptr": [0, 2, 1, 2]}),      # decreasing
    ((SC, [0, 2], 2), {"dtype": torch.float16}),
    ((SC, [0, 2], 2), {"dtype": torch.int64}),
    ((SC, [0, 2], 2), {"dtype": None}),
    ((SC, [0, 2], 2), {"fill_value": 0}),
    ((SC, [0, 2], 2), {"fill_value": -1}),
    ((SC, [0, 2], 2), {"fill_value": float("inf")}),
    ((SC, [0, 2], 2), {"fill_value": float("nan")}),
    ((SC, [0, 2], 2), {"fill_value": "1"}),
    ((SC, [0, 2], 2), {"fill_value": True}),
])
def test_snapshot_gcn_norm_bad_arguments(args, kw):
    from rlap_amd import ops
    with pytest.raises(ValueError):
        ops.snapshot_gcn_norm(*args, **kw)


def test_table_errors_are_those_of_snapshot_stats():
    from rlap_amd import ops
    for args, kw in [((SC, [0, 3], 2), {}), ((SC, [0, 2, 1, 2], 2), {}), ((SC, [0, 1, 2], 2), {"node_ptr": [0, 1, 2, 2]}),
                     ((SC, [0, 2], 2), {"node_ptr": [0, 1]})]:
        with pytest.raises(ValueError) as e1:
            ops.snapshot_stats(*args, **kw)
        with pytest.raises(ValueError) as e2:
            ops.snapshot_gcn_norm(*args, **kw)
        assert str(e1.value) == str(e2.value)


def test_valid_arguments_reach_the_device_check():
    """Well-formed arguments pass every host-side check: what stops the call on a box without a GPU is the missing device
    (RuntimeError), not a ValueError."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from rlap_amd import ops
    for kw in [{}, {"weighted": True, "dtype": torch.float64}, {"fill_value": 2}, {"node_ptr": [0, 2], "add_self_loops": False},
               {"normalize": False, "add_self_loops": False}]:
        with pytest.raises(RuntimeError):
            ops.snapshot_gcn_norm(SC, [0, 2], 2, **kw)


def test_adapters_have_the_keyword_default_off():
    from rlap_amd import adapters
    for cls in (adapters.rLap, adapters.rLapViews, adapters.rLapDepths):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["gcn_norm"].default is False and sig["fill_value"].default == 1.0, cls.__name__
    assert adapters.rLap(0.3).gcn_norm is False and adapters.rLapViews().gcn_norm is False and adapters.rLapDepths().gcn_norm is False


def test_export_flags_and_refusals_without_a_device():
    from rlap_amd import _lib
    assert "rlap_snapshot_gcn_norm" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "rlap_snapshot_gcn_norm")
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert (f"RLAP_GCN_WEIGHTED = {_lib.GCN_WEIGHTED}, RLAP_GCN_SELF_LOOPS = {_lib.GCN_SELF_LOOPS}, "
            f"RLAP_GCN_NORMALIZE = {_lib.GCN_NORMALIZE}, RLAP_GCN_F32 = {_lib.GCN_F32}") in hdr
    # a NULL handle is refused before anything else is looked at
    assert lib.rlap_snapshot_gcn_norm(None, None, 0, None, 1, None, 1, 0, 0, 1.0, None, None, None, 0, None, None) == 3

