"""The per-graph readout on the device (ops.graph_readout, rlap_readout.hip) regime by regime: what launch_readout and
launch_backward can choose (readout::dispatch, rlap_amd/csrc/rlap_readout.h) and what tests/test_gpu_readout.py does not reach.

  a. every lane count 1..32 of the staged kernel for narrow rows (k_ro_narrow), 16 bytes a lane and one element a lane, both types;
  b. rows of one wave and more (k_ro_wide): three and nine tiles of lanes, a last tile with one live lane, 64 and 200 one-element
     lanes through a misaligned view; graphs of exactly 8, 9, 16 and 17 chunks (the eight-deep loop of k_ro_finish);
  c. 40 graphs of 257 nodes: 80 of the arena's 81 slots;
  d. 40,000 small graphs and three long ones: every striding loop of the four kernels takes more than one turn of its grid;
  e. gradients: the stride-0 gradient of y.sum(), column-sliced, transposed and misaligned x;
  f. the case lists of a and b fed through readout::dispatch: every regime is reached (a condition on the lists, no measurement).

The yardsticks are those of tests/test_gpu_readout.py, without any new tolerance:
  1. independent: torch on the CPU in float64, zeros(G, F).index_add_(0, batch, x[l]); per element |y - ref| <= 2 n_g u A, u = 2^-53,
     n_g the nodes of the graph, A the sum of |x| over them; the mean adds one rounding, a float32 result 2^-24 relative; an empty
     graph is exactly +0;
  2. bit for bit: the float64 result equals the host mirror (spmm_mirror.entries on the list node i -> graph g, 1.0);
  3. a float32 result equals the mirror's float64 value of the same features rounded once.
Both are computed once per table and precision at the widest F and sliced by columns (a column's sum does not depend on the others).

A misaligned x is a contiguous view one element into a larger buffer: ops passes it on as it is, so the kernels of one element a lane
run at widths that otherwise take 16 bytes a lane.  The result buffer of ops.graph_readout comes from torch's allocator and is aligned.

Every comparison with yardstick 1 prints its largest err / bound before it asserts.  Observed on an MI355X, float64 features:
a. 0.0050 (F = 54), b. 0.0056 (F = 300, the lanes table) and 0.0016 (the long graphs), c. 0 (a graph of 257 nodes is summed in the
order of index_add_ itself), d. 0.00059.  With float32 features the ratio reaches 0.995 to 1.00 in every test: there the bound is the
one rounding to float32, 2^-24 relative, which a sum of two nodes can use up.
"""
import numpy as np
import pytest
import torch

import spmm_mirror
from test_gpu_readout import batch_of, check_stats, counts_of, mirror, ops, same_bits, table_of  # noqa: F401  (mirror, ops are fixtures)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
F64, F32 = torch.float64, torch.float32
V = {F64: 2, F32: 4}                                   # elements of a 16-byte lane
LAYERS = 2

SIZES = {
    # both sides of a piece of 8 rows, of two pieces and of a chunk; then 70 graphs of 1..5 nodes, so that a wave's 64 consecutive
    # chunks at one lane a row are all populated and split over waves; then chunked graphs behind them
    "lanes": [0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 0, 600, 2, 0] + [1 + i % 5 for i in range(70)] + [257] * 3,
    "depth": [2048, 0, 2049, 0, 4096, 0, 4097],        # 8, 9, 16 and 17 chunk sums
    "arena": [257] * 40,                               # 80 chunks, 40 chunked graphs: part_bound(10280, 40) = 81
}
TABLES = {name: table_of(s) for name, s in SIZES.items()}
FMAX = {"lanes": 513, "depth": 513, "arena": 260}


def recipe(seed, shape):
    """The features of tests/test_gpu_readout.py: mixed signs, magnitudes over ten decades, so that the order of a sum shows in its bits."""
    rng = np.random.RandomState(seed)
    return torch.from_numpy(rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-5.0, 5.0, size=shape))


def yardsticks_of(lib, node_ptr, x):
    """ref, mass (L, G, F) by torch on the CPU and the mirror's bits, of float64 features x (L, N, F)."""
    L, N, F = x.shape
    G = len(node_ptr) - 1
    batch = batch_of(node_ptr)
    ref = torch.stack([torch.zeros(G, F, dtype=F64).index_add_(0, batch, x[l]) for l in range(L)])
    mass = torch.stack([torch.zeros(G, F, dtype=F64).index_add_(0, batch, x[l].abs()) for l in range(L)])
    M = max(N, G)
    pad = np.zeros((M, F))
    bits = []
    for l in range(L):
        pad[:N] = x[l].numpy()
        bits.append(spmm_mirror.entries(lib, np.arange(N), batch.numpy(), np.ones(N), M, pad, False, False)[:G].copy())
    return {"ref": ref, "mass": mass, "mirror": torch.from_numpy(np.stack(bits))}


class Bench:
    """The features of a table and, per precision of the input, its yardsticks: made at the first use, then left unchanged."""

    def __init__(self, lib, seed, tables, fmax, layers):
        self.lib, self.seed, self.tables, self.fmax, self.layers = lib, seed, tables, fmax, layers
        self.x, self.ys = {}, {}

    def features(self, name):
        if name not in self.x:
            self.x[name] = recipe(self.seed + len(self.x), (self.layers, self.tables[name][-1], self.fmax[name]))
        return self.x[name]

    def yardsticks(self, name, dtype):
        if (name, dtype) not in self.ys:
            x = self.features(name)
            self.ys[name, dtype] = yardsticks_of(self.lib, self.tables[name], x if dtype == F64 else x.float().double())
        return self.ys[name, dtype]


@pytest.fixture(scope="module")
def bench(mirror):
    return Bench(mirror, 21, TABLES, FMAX, LAYERS)


def on_device(values, aligned):
    """`values` (a CPU tensor) on the device: from torch's allocator, or a contiguous view one element into a larger buffer."""
    if aligned:
        x = values.contiguous().cuda()
        assert x.data_ptr() % 16 == 0
        return x
    count = values.numel()
    big = torch.empty(count + 8, dtype=values.dtype, device="cuda")
    assert big.data_ptr() % 16 == 0
    big[1:1 + count] = values.reshape(-1).cuda()
    x = big[1:1 + count].view(values.shape)
    # the conditions of the case: without them it tests nothing
    assert x.is_contiguous() and x.data_ptr() % 16 != 0 and x.data_ptr() % x.element_size() == 0
    assert x.detach().to(device=x.device).contiguous().data_ptr() == x.data_ptr(), "the view is passed on as it is"
    return x


def compare(what, y, ys, node_ptr, reduce):
    """y (L, G, F) of float64 or float32 features against the three yardsticks, sliced to its shape."""
    L, G, F = y.shape
    n = counts_of(node_ptr)[None, :, None]
    div = n.clamp_min(1.0) if reduce == "mean" else torch.ones_like(n)
    ref, mass, bits = ys["ref"][:L, :, :F] / div, ys["mass"][:L, :, :F] / div, ys["mirror"][:L, :, :F] / div
    bound = 2 * n * U * mass + (U * ref.abs() if reduce == "mean" else 0)
    if y.dtype == F32:
        bound = bound + 2.0 ** -24 * (ref.abs() + bound)
    err = (y.cpu().double() - ref).abs()
    print(f"{what} {reduce}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= bound).all()), what
    assert same_bits(y, bits if y.dtype == F64 else bits.float()), f"{what}: not the mirror's bits"
    empty = n[0, :, 0] == 0
    assert same_bits(y[:, empty.cuda()], torch.zeros(L, int(empty.sum()), F, dtype=y.dtype)), f"{what}: an empty graph is not +0"


def run_case(ops, bench, name, dtype, F, aligned, reduces=("sum",), poison=False):
    node_ptr = TABLES[name]
    G = len(node_ptr) - 1
    x = on_device(bench.features(name)[:, :, :F].to(dtype), aligned)
    ys = bench.yardsticks(name, dtype)
    what = f"{name} {str(dtype)[6:]} F={F} {'aligned' if aligned else 'misaligned'}"
    for reduce in reduces:
        y = ops.graph_readout(x, node_ptr, reduce=reduce)
        check_stats(ops, node_ptr)
        assert y.shape == (LAYERS, G, F) and y.dtype == dtype and y.is_cuda and y.data_ptr() % 16 == 0
        compare(what, y, ys, node_ptr, reduce)
        if poison:
            ops.debug_set_poison(0xA5)
            try:
                assert same_bits(y, ops.graph_readout(x, node_ptr, reduce=reduce)), f"{what}: depends on what the arena or y held"
            finally:
                ops.debug_set_poison(-1)
    return x


# ------------------------------------------------------------------------------------------------ a. the lanes of the narrow kernel
def narrow_case(dtype, mode, lanes):
    """(F, aligned): 16 bytes a lane is F = V lanes on aligned x; one element a lane is F = lanes, misaligned where F is a multiple of V."""
    if mode == "vector":
        return V[dtype] * lanes, True
    return lanes, lanes % V[dtype] != 0


NARROW = [(dtype, mode, lanes) for dtype in (F32, F64) for mode in ("vector", "scalar") for lanes in range(1, 33)]
MEAN_LANES = (2, 5, 7, 13, 31)
POISON_LANES = (2, 7, 13)


@pytest.mark.parametrize("dtype,mode,lanes", NARROW, ids=[f"{str(d)[6:]}-{m}-{n}" for d, m, n in NARROW])
def test_narrow_lane_sweep(ops, bench, dtype, mode, lanes):
    F, aligned = narrow_case(dtype, mode, lanes)
    reduces = ("sum", "mean") if lanes in MEAN_LANES else ("sum",)
    run_case(ops, bench, "lanes", dtype, F, aligned, reduces, poison=lanes in POISON_LANES)


# ------------------------------------------------------------------------------------------------ b. wide rows, long graphs
WIDE = [
    (F64, 129, True),     # one element a lane, three tiles, the last with one live lane
    (F64, 300, True),     # 16 bytes a lane, 150 lanes, three tiles
    (F32, 260, True),     # 16 bytes a lane, 65 lanes, two tiles, the last with one live lane
    (F32, 513, True),     # one element a lane, nine tiles, the last with one live lane
    (F32, 200, False), (F64, 200, False),   # 200 one-element lanes: four tiles
    (F32, 64, False), (F64, 64, False),     # 64 one-element lanes: one full tile
    (F32, 200, True),     # 16 bytes a lane, 50 lanes: one tile with idle lanes
    (F64, 65, True),      # one element a lane, two tiles, the last with one live lane
]
DEPTH_NARROW = [(F32, 20, True), (F64, 7, True)]      # 5 lanes of 16 bytes; 7 one-element lanes


@pytest.mark.parametrize("name", ["lanes", "depth"])
@pytest.mark.parametrize("dtype,F,aligned", WIDE, ids=[f"{str(d)[6:]}-{F}-{'aligned' if a else 'misaligned'}" for d, F, a in WIDE])
def test_wide_tiles(ops, bench, name, dtype, F, aligned):
    run_case(ops, bench, name, dtype, F, aligned, ("sum", "mean"))


@pytest.mark.parametrize("dtype,F,aligned", DEPTH_NARROW, ids=["float32-20", "float64-7"])
def test_long_graphs_narrow(ops, bench, dtype, F, aligned):
    sizes = np.diff(TABLES["depth"])
    assert sorted(((sizes + 255) // 256)[sizes > 0].tolist()) == [8, 9, 16, 17]
    run_case(ops, bench, "depth", dtype, F, aligned, ("sum", "mean"), poison=True)


# ------------------------------------------------------------------------------------------------ c. the arena near its bound
@pytest.mark.parametrize("dtype,F,aligned", [(F32, 24, True), (F32, 260, True), (F64, 9, True), (F64, 129, True)],
                         ids=["float32-24", "float32-260", "float64-9", "float64-129"])
def test_arena_near_its_bound(ops, bench, dtype, F, aligned):
    node_ptr = TABLES["arena"]
    N, G = node_ptr[-1], len(node_ptr) - 1
    assert (N + 255) // 256 + min(G, N // 257) == 81           # readout::part_bound: the slots of the arena
    for reduce in ("sum", "mean"):
        run_case(ops, bench, "arena", dtype, F, aligned, (reduce,), poison=True)
        assert ops.last_stats["chunks"] == 80 and ops.last_stats["chunked_graphs"] == 40


# ------------------------------------------------------------------------------------------------ d. grids that stride
# 40,000 graphs of 0 to 3 nodes, then three long ones and an empty last one.  (The graph of 20,000 nodes makes the gather of the
# float64 case, 32 units a row, longer than one turn of its grid as well.)
MANY_SIZES = [(0, 1, 2, 3, 0, 1)[i % 6] for i in range(40000)] + [20000, 3000, 257, 0]
MANY = table_of(MANY_SIZES)
MANY_L, MANY_F = 3, 65
RO_MAX_GRID, RO_WAVES, RO_THREADS = 8192, 4, 256       # rlap_readout.hip: workgroups of a launch, waves and threads of a workgroup
STRIDING = [(F32, 65), (F64, 64)]


@pytest.fixture(scope="module")
def many(mirror):
    return Bench(mirror, 33, {"many": MANY}, {"many": MANY_F}, MANY_L)


@pytest.mark.parametrize("dtype,F", STRIDING, ids=["float32-65-wide", "float64-64-narrow"])
def test_striding_grids(ops, mirror, many, dtype, F):
    node_ptr = MANY
    N, G, L = node_ptr[-1], len(node_ptr) - 1, MANY_L
    sizes = np.diff(node_ptr)
    chunks = int(((sizes + 255) // 256).sum())
    # before any device call: every kernel of this case has more work than one turn of its grid.  The grid is sized from the bound
    # ceil(N / 256) + G and capped at RO_MAX_GRID = 8192 workgroups of RO_WAVES = 4 waves, RO_THREADS = 256 threads; the kernels
    # stride to the true counts, which are the smaller ones.
    d = spmm_mirror.readout_dispatch(mirror, F, 4 if dtype == F32 else 8, True)
    bound = (N + 255) // 256 + G
    if dtype == F32:
        assert (d["vec"], d["lg"], d["ftiles"]) == (False, 6, 2)
        items, sized = L * chunks * d["ftiles"], L * bound * d["ftiles"]  # k_ro_wide: (layer, chunk, feature tile)
    else:
        assert (d["vec"], d["lg"], d["lanes"]) == (True, 5, 32)
        per_wave = 64 >> d["lg"]                                          # k_ro_narrow: (layer, two chunks)
        items, sized = L * ((chunks + per_wave - 1) // per_wave), L * ((bound + per_wave - 1) // per_wave)
    assert sized >= items > RO_MAX_GRID * RO_WAVES
    assert L * G * F > RO_MAX_GRID * RO_THREADS                          # k_ro_finish: elements of y
    assert N * d["lanes"] > RO_MAX_GRID * RO_THREADS                      # k_ro_backward: N x F / VEC units (gy and gx are aligned)
    assert sizes[-1] == 0 and sizes[-2] > 256 and sizes[-4] > 256         # what the finish kernel's later turns must write

    xc = many.features("many")[:, :, :F].to(dtype)
    ys = many.yardsticks("many", dtype)
    batch, n = batch_of(node_ptr), counts_of(node_ptr)
    gy = xc[:, :G].contiguous().cuda()                                    # (any values serve as the gradient of y)
    for reduce in ("sum", "mean"):
        x = on_device(xc, True).requires_grad_(True)
        y = ops.graph_readout(x, node_ptr, reduce=reduce)
        check_stats(ops, node_ptr)
        compare(f"many {str(dtype)[6:]} F={F}", y.detach(), ys, node_ptr, reduce)      # (checks y[:, empty] is exactly +0)
        yc = y.detach().cpu()
        for g in (G - 4, G - 3, G - 2):                                   # the long graphs, element by element
            s, e = node_ptr[g], node_ptr[g + 1]
            for l in (0, L - 1):
                for f in (0, 31, F - 1):
                    want = spmm_mirror.list_sum(mirror, np.ones(e - s), xc[l, s:e, f].double().numpy())
                    if reduce == "mean":
                        want = want / np.float64(e - s)
                    want = want.astype(np.float32 if dtype == F32 else np.float64)
                    assert yc[l, g, f].numpy().tobytes() == want.tobytes(), (reduce, g, l, f)
        y.backward(gy)
        assert ops.last_stats["host_syncs"] == 0 and ops.last_stats["rows"] == N
        want = gy.cpu()[:, batch]
        if reduce == "mean":
            want = (want.double() / n[batch][None, :, None]).to(dtype)    # one float64 division, rounded once
        assert same_bits(x.grad, want), f"{reduce}: the gradient is not the gather"


# ------------------------------------------------------------------------------------------------ e. gradients
GRADS = [(F32, 28), (F32, 260), (F64, 13), (F64, 129)]


def gather(gy, node_ptr, reduce):
    batch, n = batch_of(node_ptr), counts_of(node_ptr)
    want = gy.cpu()[:, batch]
    if reduce == "mean":
        want = (want.double() / n[batch][None, :, None]).to(gy.dtype)      # one float64 division, rounded once
    return want


@pytest.mark.parametrize("dtype,F", GRADS, ids=[f"{str(d)[6:]}-{F}" for d, F in GRADS])
def test_gradients(ops, bench, dtype, F):
    node_ptr = TABLES["lanes"]
    N, G = node_ptr[-1], len(node_ptr) - 1
    xc = bench.features("lanes")[:, :, :F].to(dtype).contiguous()
    gy = bench.features("lanes")[:, :G, 100:100 + F].to(dtype).contiguous().cuda()
    for reduce in ("sum", "mean"):
        plain = ops.graph_readout(xc.cuda(), node_ptr, reduce=reduce)
        # the gradient of y.sum(): expanded, every stride 0
        x = xc.cuda().requires_grad_(True)
        ops.graph_readout(x, node_ptr, reduce=reduce).sum().backward()
        assert same_bits(x.grad, gather(torch.ones(LAYERS, G, F, dtype=dtype), node_ptr, reduce)), f"{reduce}: y.sum()"
        # x every second column of a wider tensor
        big = torch.zeros(LAYERS, N, 2 * F, dtype=dtype, device="cuda")
        big[:, :, ::2] = xc.cuda()
        big.requires_grad_(True)
        x = big[:, :, ::2]
        assert not x.is_contiguous()
        y = ops.graph_readout(x, node_ptr, reduce=reduce)
        assert same_bits(y, plain)
        y.backward(gy)
        assert same_bits(big.grad[:, :, ::2], gather(gy, node_ptr, reduce)), f"{reduce}: column-sliced x"
        assert same_bits(big.grad[:, :, 1::2], torch.zeros(LAYERS, N, F, dtype=dtype))
        # x the transpose of an (L, F, N) tensor
        base = xc.transpose(1, 2).contiguous().cuda().requires_grad_(True)
        x = base.transpose(1, 2)
        assert x.shape == (LAYERS, N, F) and not x.is_contiguous()
        y = ops.graph_readout(x, node_ptr, reduce=reduce)
        assert same_bits(y, plain)
        y.backward(gy)
        assert same_bits(base.grad.transpose(1, 2), gather(gy, node_ptr, reduce)), f"{reduce}: transposed x"
        # x contiguous and misaligned
        x = on_device(xc, False).requires_grad_(True)
        y = ops.graph_readout(x, node_ptr, reduce=reduce)
        assert x.data_ptr() % 16 != 0 and same_bits(y, plain)
        y.backward(gy)
        assert same_bits(x.grad, gather(gy, node_ptr, reduce)), f"{reduce}: misaligned x"


# ------------------------------------------------------------------------------------------------ f. which regimes a and b reach
def test_the_cases_reach_every_regime(mirror):
    """No device call: every (type, F, aligned) of a and b through readout::dispatch, the rule both launchers call."""
    def regime(dtype, F, aligned):
        return spmm_mirror.readout_dispatch(mirror, F, 4 if dtype == F32 else 8, aligned)

    narrow = set()
    for dtype, mode, lanes in NARROW:
        F, aligned = narrow_case(dtype, mode, lanes)
        d = regime(dtype, F, aligned)
        assert d["lg"] < 6 and d["ftiles"] == 1 and d["vec"] == (mode == "vector") and d["lanes"] == lanes, (dtype, mode, lanes, d)
        assert (1 << d["lg"]) >= lanes > (1 << d["lg"]) // 2 or lanes == 1
        narrow.add((dtype, d["vec"], d["lanes"]))
    assert narrow == {(dtype, vec, lanes) for dtype in (F32, F64) for vec in (True, False) for lanes in range(1, 33)}
    for dtype, F, aligned in DEPTH_NARROW:
        assert regime(dtype, F, aligned)["lg"] < 6

    wide, one_live_lane = {}, 0
    for dtype, F, aligned in WIDE:
        d = regime(dtype, F, aligned)
        assert d["lg"] == 6 and d["lanes"] > 32, (dtype, F, aligned, d)
        wide.setdefault((d["vec"], min(d["ftiles"], 3)), set()).add(dtype)
        one_live_lane += d["lanes"] % 64 == 1
    assert set(wide) == {(vec, tiles) for vec in (True, False) for tiles in (1, 2, 3)}, sorted(wide)
    assert one_live_lane >= 1
    for dtype, F in STRIDING:                                              # d runs one kernel each
        assert regime(dtype, F, True)["lg"] == (6 if dtype == F32 else 5)
