"""Device-native augmentor adapters.

Mirrors of the reference's L2 adapters that keep everything on the GPU:
  * `rLap`     -- PyGCL-style augmentor, scripts/augmentor_benchmarks.py:68-96
  * `rLapDGL`  -- DGL-style augmentor, CCA-SSG/aug.py:33-63
  * `rLapViews` -- K rLap views of one graph from one library call, with PyGCL-style
                  siblings for the `(aug1, aug2)` pair of scripts/node_shared.py:488-498
  * `rLapDepths` -- the same graph at K removed fractions from one elimination
                  (the sweeps of scripts/rlap_vc_spectral.py, scripts/rlap_ppr_edge_plots.py); `.diffuse`
                  gives their PPR diffusions from one ops.snapshot_ppr call, `.relabelled` their compact graphs and id maps and
                  `.batch_edge_counts` the batch subgraph sizes from ops.snapshot_subgraph
  * `gcn_norm=True` on rLap / rLapViews / rLapDepths: the graphs come with self loops and GCN coefficients from one
                  ops.snapshot_gcn_norm call, for GCNConv(..., normalize=False)
  * `.snapshots(g)` on rLap / rLapViews / rLapDepths: the same one elimination call as a `Snapshots` holder, whose `.propagate(x)`
                  is the sparse product of a GCN layer for all views at once (ops.snapshot_propagate); `SnapshotGCNConv` is the
                  layer built on it
  * graph-level steps (scripts/graph_shared.py): `node_ptr_of(batch)` turns a PyG `batch` vector into the `node_ptr` of a batch;
                  `.snapshots(g, node_ptr=)` on rLapViews / rLapDepths eliminates every graph of the batch in the one call;
                  `Snapshots.aggregate(x)` is GIN's plain neighbour sum, `SnapshotGINConv` the layer on it, and
                  `Snapshots.readout(z)` the per-graph sum of global_add_pool (ops.graph_readout)
  * `NodeContrast` -- the contrastive loss of the node-level step (scripts/node_shared.py: DualBranchContrast(InfoNCEBatched(tau),
                  mode="L2L")) on the embeddings of two views, fused on the device (ops.info_nce)
  * `CCAContrast` -- the loss of CCA-SSG/main.py on the embeddings of two views, fused on the device (ops.cca_loss);
                  `drop_feature` -- CCA-SSG/aug.py's feature masking (also A.FeatureMasking), one mask per view
  * `BarlowTwinsContrast` -- PyGCL's WithinEmbedContrast(L.BarlowTwins()) on the embeddings of two views, fused on the device
                  (ops.barlow_twins_loss)
  * `SnapshotBatchNorm` -- BatchNorm1d for all views of a call at once, each view with its own statistics, the activations around
                  it fused in (ops.batch_norm); `SnapshotGINEncoder` -- scripts/graph_shared.py's GConv on a `Snapshots`: GIN layer,
                  relu + norm, readout, per layer
  * `rLapChain` -- the chain of scripts/rlap_vc_spectral.py: eliminate, relabel the survivors 0..k-1, eliminate again
  * `EdgeDropping`, `EdgeDroppingDegree`, `EdgeDroppingPR`, `EdgeDroppingEVC` -- the comparison arms of
                  scripts/augmentor_benchmarks.py:216-363 on the device (ops.drop_edges); `EdgeDroppingViews` -- K of them from one call
  * `NodeDropping`, `RWSampling` -- PyGCL's node-sampling arms (scripts/node_shared.py:458-470) on the device
                  (ops.sample_subgraphs); `NodeSampleViews` -- K of them from one call
  * `EdgeAdding` -- the reference's own edge-adding arm (scripts/augmentor_benchmarks.py:44-65) on the device (ops.add_edges);
                  `EdgeAddingViews` -- K of them from one call, the input sorted once at most
PyGCL / DGL are optional: with them installed the classes return their graph types,
without them a small named tuple with the same fields.
"""
from collections import namedtuple
from typing import Optional

import torch

from . import ops

Graph = namedtuple("Graph", ["x", "edge_index", "edge_weights"])


def _schur(edge_index, edge_weights, x, frac, o_v, o_n, seed, num_nodes_from_x, symmetrize):
    """One call of the op the way the reference adapters make it: num_nodes = edge_index.max() + 1 and
    num_remove = int(frac * num_nodes) (scripts/augmentor_benchmarks.py:77-78), both found inside the C ABI
    (no torch reduction, no `.item()`).  `num_nodes_from_x=True` is the explicit opt-in to x.shape[0] instead
    (differs from the reference when the trailing nodes are isolated: more vertices enter the queue)."""
    n = int(x.shape[0]) if (num_nodes_from_x and x is not None) else None
    return ops.approximate_cholesky_from_edges(edge_index, edge_weights, n, None, o_v, o_n, remove_frac=frac,
                                               symmetrize=symmetrize, seed=seed, return_device="same")


class Snapshots:
    """The snapshots of one elimination call as the propagation takes them: (sc, ptr, num_nodes, node_ptr, weighted, fill_value).
    `.propagate(x)` is A^ x for every layer at once (ops.snapshot_propagate with self loops and the GCN normalisation -- the list
    `gcn_norm=True` hands to GCNConv(..., normalize=False), never written out); `transpose=True` the transposed product."""

    def __init__(self, sc, ptr, num_nodes: int, node_ptr=None, weighted: bool = False, fill_value: float = 1.0):
        self.sc, self.ptr, self.num_nodes, self.node_ptr = sc, ptr, int(num_nodes), node_ptr
        self.weighted, self.fill_value = bool(weighted), fill_value
        self._table = None   # (the readout's ops.GraphTable, made on first use)

    @property
    def layers(self) -> int:
        graphs = 1 if self.node_ptr is None else len(self.node_ptr) - 1
        return (len(self.ptr) - 1) // graphs

    def propagate(self, x, transpose: bool = False):
        return ops.snapshot_propagate(self.sc, self.ptr, self.num_nodes, x, node_ptr=self.node_ptr, weighted=self.weighted,
                                      add_self_loops=True, fill_value=self.fill_value, normalize=True, transpose=transpose)

    def aggregate(self, x, transpose: bool = False):
        """GIN's aggregation for every layer at once: y[l, i] = the sum of x[j] over the neighbours j of i in snapshot l -- the
        product without self loops and without the normalisation (weights kept iff the holder's `weighted`)."""
        return ops.snapshot_propagate(self.sc, self.ptr, self.num_nodes, x, node_ptr=self.node_ptr, weighted=self.weighted,
                                      add_self_loops=False, fill_value=self.fill_value, normalize=False, transpose=transpose)

    def readout(self, z, reduce: str = "sum"):
        """global_add_pool (reduce="mean": global_mean_pool) of node embeddings z, (n, F) or (L, n, F), over the holder's batch:
        ops.graph_readout with its `node_ptr`, (G, F) or (L, G, F).  Without a `node_ptr` the whole id range is one graph.  The
        table is checked and copied to the device once and kept on the holder."""
        if self._table is None:
            self._table = ops.GraphTable([0, self.num_nodes] if self.node_ptr is None else self.node_ptr, self.num_nodes)
        return ops.graph_readout(z, self._table, reduce=reduce)

    def plan(self, directions: str = "both") -> "PlannedSnapshots":
        """The same snapshots served by one propagation plan (ops.snapshot_plan), built on first use: for the six to twelve
        products a training step makes on them.  SnapshotGCNConv takes the holder as it takes this one."""
        return PlannedSnapshots(self, directions)


class PlannedSnapshots:
    """`Snapshots` behind a plan: the same `.layers` and `.propagate(x, transpose=False)`, the same bits, the lists built once (on
    the first product) instead of in every call.  `snapshot_plan` is the ops.SnapshotPlan, None before the first use."""

    def __init__(self, snapshots: Snapshots, directions: str = "both"):
        if directions not in ops.PLAN_DIRECTIONS:
            raise ValueError(f"directions: one of {sorted(ops.PLAN_DIRECTIONS)}, got {directions!r}")
        self.snapshots, self.directions, self.snapshot_plan = snapshots, directions, None
        self.aggregate_plan = None   # (the second plan, of `aggregate`: no loops, no normalisation; None before its first use)

    @property
    def layers(self) -> int:
        return self.snapshots.layers

    @property
    def num_nodes(self) -> int:
        return self.snapshots.num_nodes

    def propagate(self, x, transpose: bool = False):
        if self.snapshot_plan is None:
            s = self.snapshots
            self.snapshot_plan = ops.snapshot_plan(s.sc, s.ptr, s.num_nodes, node_ptr=s.node_ptr, weighted=s.weighted, add_self_loops=True,
                                                   fill_value=s.fill_value, normalize=True, directions=self.directions)
        return self.snapshot_plan.propagate(x, transpose=transpose)

    def aggregate(self, x, transpose: bool = False):
        """`Snapshots.aggregate` over a second plan with its flags (no self loops, no normalisation), built on first use."""
        if self.aggregate_plan is None:
            s = self.snapshots
            self.aggregate_plan = ops.snapshot_plan(s.sc, s.ptr, s.num_nodes, node_ptr=s.node_ptr, weighted=s.weighted, add_self_loops=False,
                                                    fill_value=s.fill_value, normalize=False, directions=self.directions)
        return self.aggregate_plan.propagate(x, transpose=transpose)

    def readout(self, z, reduce: str = "sum"):
        return self.snapshots.readout(z, reduce=reduce)


def node_ptr_of(batch, num_graphs: Optional[int] = None) -> torch.Tensor:
    """The `node_ptr` of a PyG `batch` vector (batch[i] = the graph of node i, sorted, as DataLoader collates it): an int64 CPU
    table [G+1] with node_ptr[g] the first node of graph g.  G is `num_graphs`, or batch.max() + 1.  bincount and cumsum on
    batch's device, then ONE read by the host.  A vector that is not sorted, holds a negative entry or an entry >= num_graphs
    raises ValueError."""
    b = torch.as_tensor(batch)
    if b.dim() != 1 or b.dtype.is_floating_point or b.dtype.is_complex or b.dtype == torch.bool:
        raise ValueError("batch: a 1-D vector of graph numbers")
    if num_graphs is not None and (isinstance(num_graphs, bool) or not hasattr(num_graphs, "__index__") or num_graphs.__index__() < 0):
        raise ValueError(f"num_graphs: a non-negative integer, got {num_graphs!r}")
    G = None if num_graphs is None else num_graphs.__index__()
    b = b.to(torch.int64)
    bad = (b[1:] < b[:-1]).any() | (b[:1] < 0).any()
    counts = torch.bincount(b.clamp_min(0), minlength=G or 0)
    table = torch.cat([bad.reshape(1).to(torch.int64), torch.zeros(1, dtype=torch.int64, device=b.device), counts.cumsum(0)]).cpu()
    if int(table[0]):
        raise ValueError("batch: not sorted (node_ptr needs the nodes of a graph side by side), or a negative entry")
    if G is not None and table.numel() - 2 > G:
        raise ValueError(f"batch: an entry >= num_graphs ({G})")
    return table[1:].contiguous()


def _batch_tables(node_ptr, x, fracs):
    """`node_ptr` checked (ops._ptr_table), the batch's num_nodes and, per fraction, int(frac * n_g) for every graph g."""
    np_ = ops._ptr_table(node_ptr, "node_ptr", 0, None)
    n = int(np_[-1])
    if x is not None and int(x.shape[0]) != n:
        raise ValueError(f"x: {int(x.shape[0])} rows, node_ptr[-1] is {n}")
    sizes = (np_[1:] - np_[:-1]).tolist()
    return np_, n, [[int(f * n_g) for n_g in sizes] for f in fracs]


def _snapshots_of(x, sc, ptr, num_nodes, keep_weights, fill_value):
    """The holder of one call; like _gcn_graphs the loops cover x.shape[0] nodes when x is given, else the call's num_nodes."""
    return Snapshots(sc, ptr, int(x.shape[0]) if x is not None else int(num_nodes), None, keep_weights, fill_value)


def _dense_arg(dense) -> str:
    if dense not in ("torch", "device"):
        raise ValueError(f'dense: "torch" or "device", got {dense!r}')
    return dense


class SnapshotLinear(torch.nn.Module):
    """torch.nn.Linear with a fused activation, on the device: forward(x) = ops.linear_act(x, weight, bias, act, alpha,
    weight_layout="out_in") for x (N, in_features) or (L, N, in_features) -- one pass over x instead of the matmul, the bias add and
    the activation.  Parameter names, shapes and initialisation are torch.nn.Linear's (`weight` is
    (out_features, in_features), read in place in that layout; `bias` (out_features,) or None), so a Linear's state dict loads.
    `act` is "none", "relu" or "elu" (`alpha` is ELU's)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, act: str = "none", alpha: float = 1.0):
        super().__init__()
        if act not in ops.LINEAR_ACT:
            raise ValueError(f"act: one of {sorted(ops.LINEAR_ACT)}, got {act!r}")
        self.in_features, self.out_features, self.act, self.alpha = int(in_features), int(out_features), act, float(alpha)
        self.weight = torch.nn.Parameter(torch.empty(self.out_features, self.in_features))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(self.out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.Linear.reset_parameters(self)   # (reads weight, bias and weight's shape alone)

    def forward(self, x):
        return ops.linear_act(x, self.weight, self.bias, act=self.act, alpha=self.alpha, weight_layout="out_in")

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, act={self.act!r}"


class SnapshotMLP(torch.nn.Module):
    """Linear -> act -> Linear in two device calls, the first with the activation fused: the `nn` of scripts/graph_shared.py's GIN
    layers, nn.Sequential(Linear(in, hidden), ReLU(), Linear(hidden, hidden)), and CCA-SSG/model.py's MLP without its batch norm
    (use_bn=False).  The two layers are `fc1` and `fc2`, SnapshotLinears; forward(x) takes (N, in_dim) or (L, N, in_dim)."""

    def __init__(self, in_dim: int, hidden_dim: int, out_dim: int, act: str = "relu"):
        super().__init__()
        self.fc1 = SnapshotLinear(in_dim, hidden_dim, act=act)
        self.fc2 = SnapshotLinear(hidden_dim, out_dim)

    def forward(self, x):
        return self.fc2(self.fc1(x))


class ProjectionHead(SnapshotMLP):
    """scripts/node_shared.py's `project`: fc2(F.elu(fc1(z))) with fc1 = Linear(hidden_dim, proj_dim) and
    fc2 = Linear(proj_dim, hidden_dim), the ELU fused into the first call."""

    def __init__(self, hidden_dim: int, proj_dim: int, act: str = "elu"):
        super().__init__(hidden_dim, proj_dim, hidden_dim, act=act)


def _gin_mlp(d: int, hidden_dim: int, dense: str) -> torch.nn.Module:
    """The MLP of a GIN layer: torch's modules, or with dense="device" the fused SnapshotMLP."""
    if dense == "device":
        return SnapshotMLP(d, hidden_dim, hidden_dim)
    return torch.nn.Sequential(torch.nn.Linear(d, hidden_dim), torch.nn.ReLU(), torch.nn.Linear(hidden_dim, hidden_dim))


class SnapshotGCNConv(torch.nn.Module):
    """GCNConv for all views of a call at once: forward(x, snapshots) = snapshots.propagate(x @ W) + b, an (L, n, out_channels)
    tensor for the L layers of `snapshots` (a `Snapshots`).  x is (n, in_channels), shared by the layers (the first GCN layer of
    every view), or (L, n, in_channels) (the later ones).  The dense product is torch's, the sparse one ops.snapshot_propagate;
    gradients reach W, b and x.  `snapshots` is taken by duck typing: anything with `.propagate(x, transpose=False)` and the
    (L, n, F) result serves, so forward(x, plan) with an ops.SnapshotPlan -- graph_plan(g) for the input graph itself,
    rLapDepths.diffuse_plan(g) for its PPR diffusions -- works as it does with a holder.  Glorot-uniform W and zero b, as PyG's GCNConv initialises them.  (Unpinned: PyG is not installed
    here; this restates its published semantics -- linear without bias, propagate with gcn_norm's coefficients, then the bias --
    not a run of it: DESIGN 4.10 and section 7.)

    The first layer also takes an ops.FeaturePlan as x: forward(fp, snapshots, keep) = snapshots.propagate(fp.linear(W, keep)) + b,
    with `keep` None (every layer reads x @ W) or the (K, in_channels) masks of ops.feature_masks, one view per layer
    (DESIGN 4.26); gradients then reach W and b.

    `epilogue`, a SnapshotActDropout, makes the layer return epilogue(propagate(x @ W), b): the bias add, the activation and the
    dropout of scripts/node_shared.py's `GCNConv -> PReLU` in one fused pass.  Without it the layer is what it was.

    `dense="device"` computes x @ W by ops.linear_act, so that every value of the layer has a stated order; the
    default "torch" leaves the product to torch, as before."""

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True, epilogue=None, dense: str = "torch"):
        super().__init__()
        self.dense = _dense_arg(dense)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.weight = torch.nn.Parameter(torch.empty(self.in_channels, self.out_channels))
        self.bias = torch.nn.Parameter(torch.empty(self.out_channels)) if bias else None
        if epilogue is not None and not isinstance(epilogue, SnapshotActDropout):
            raise ValueError("SnapshotGCNConv: epilogue is a SnapshotActDropout or None")
        self.epilogue = epilogue
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x, snapshots: Snapshots, keep=None):
        if isinstance(x, ops.FeaturePlan):   # the sparse first layer: every view's (x * keep[k]) @ W from the plan's lists
            y = snapshots.propagate(x.linear(self.weight, keep))
        elif keep is not None:
            raise ValueError("SnapshotGCNConv: keep goes with an ops.FeaturePlan as x (mask a tensor x with drop_feature)")
        elif self.dense == "device":
            y = snapshots.propagate(ops.linear_act(x, self.weight))
        else:
            y = snapshots.propagate(x @ self.weight)
        if self.epilogue is not None:
            return self.epilogue(y, self.bias)
        return y if self.bias is None else y + self.bias


class SnapshotGINConv(torch.nn.Module):
    """GINConv for all views of a call at once: forward(x, snapshots) = nn((1 + eps) * x + snapshots.aggregate(x)), an
    (L, n, out) tensor for the L layers of `snapshots`.  x is (n, F), shared by the layers (the first GIN layer of every view), or
    (L, n, F) (the later ones); `nn` is any module mapping (..., F) to (..., out), the MLP of scripts/graph_shared.py.  `eps` is a
    parameter when `train_eps` is set, else a buffer.  The neighbour sum is ops.snapshot_propagate without loops and without the
    normalisation, in its fixed order; gradients reach nn, eps and x.  `snapshots` is taken by duck typing: anything with
    `.aggregate(x)` and the (L, n, F) result serves -- a `Snapshots`, or its `.plan()`.  (Unpinned: PyG is not installed here; this
    restates its published semantics -- x_i' = nn((1 + eps) x_i + sum_j x_j) -- not a run of it.)"""

    def __init__(self, nn: torch.nn.Module, eps: float = 0.0, train_eps: bool = False):
        super().__init__()
        self.nn, self.initial_eps = nn, float(eps)
        if train_eps:
            self.eps = torch.nn.Parameter(torch.empty(()))
        else:
            self.register_buffer("eps", torch.empty(()))
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            self.eps.fill_(self.initial_eps)
        for m in self.nn.modules():
            if m is not self.nn and hasattr(m, "reset_parameters"):
                m.reset_parameters()
        if hasattr(self.nn, "reset_parameters"):
            self.nn.reset_parameters()

    def forward(self, x, snapshots):
        return self.nn((1 + self.eps).to(x.dtype) * x + snapshots.aggregate(x))


class SnapshotBatchNorm(torch.nn.Module):
    """BatchNorm1d for all views of a call at once: forward(x) = ops.batch_norm on an (L, N, F) tensor (or one (N, F) view), every
    layer normalised with its own batch statistics and the running buffers updated once a layer, the layers in order.  That one
    view per layer and view-ordered buffer updates is the reference's behaviour: scripts/graph_shared.py and
    scripts/graph_shared_g2l.py run their encoders once per view, so torch.nn.BatchNorm1d sees one view a call; on an (L, N, F)
    tensor it would take dim 1 for the channels, and on the (L * N, F) reshape it would mix the views' statistics.  `pre="relu"`
    fuses the F.relu in front (GConv: conv -> relu -> bn), `post="relu"` / `"prelu"` the activation behind (the projection head and
    the predictor: Linear -> BatchNorm1d -> PReLU); with `"prelu"` the module carries the slope as the parameter `slope`
    (`slope_init`, one value or `slope_per_channel`).  It restates torch.nn.BatchNorm1d's published semantics -- parameter and
    buffer names `weight`, `bias`, `running_mean`, `running_var`, `num_batches_tracked`, so a state dict moves across; ones and
    zeros at reset; `.train()` / `.eval()`; without `track_running_stats` batch statistics in both modes -- except
    `momentum=None`, the cumulative average, which is refused.  `num_batches_tracked` grows by L a call (host arithmetic)."""

    def __init__(self, num_features: int, eps: float = 1e-5, momentum: float = 0.1, affine: bool = True, track_running_stats: bool = True,
                 pre: str = "none", post: str = "none", slope_init: float = 0.25, slope_per_channel: bool = False):
        super().__init__()
        if momentum is None:
            raise ValueError("momentum: a number in [0, 1]; the cumulative average (momentum=None) is not provided")
        if pre not in ops.NORM_PRE or post not in ops.NORM_POST:
            raise ValueError(f"pre: one of {sorted(ops.NORM_PRE)}; post: one of {sorted(ops.NORM_POST)}")
        self.num_features, self.eps, self.momentum = int(num_features), eps, momentum
        self.affine, self.track_running_stats, self.pre, self.post = bool(affine), bool(track_running_stats), pre, post
        self.slope_init = float(slope_init)
        if self.affine:
            self.weight = torch.nn.Parameter(torch.empty(self.num_features))
            self.bias = torch.nn.Parameter(torch.empty(self.num_features))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        if self.track_running_stats:
            self.register_buffer("running_mean", torch.zeros(self.num_features))
            self.register_buffer("running_var", torch.ones(self.num_features))
            self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        else:
            self.register_buffer("running_mean", None)
            self.register_buffer("running_var", None)
            self.register_buffer("num_batches_tracked", None)
        if post == "prelu":
            self.slope = torch.nn.Parameter(torch.empty(self.num_features if slope_per_channel else 1))
        else:
            self.register_parameter("slope", None)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            if self.track_running_stats:
                self.running_mean.zero_()
                self.running_var.fill_(1.0)
                self.num_batches_tracked.zero_()
            if self.affine:
                self.weight.fill_(1.0)
                self.bias.zero_()
            if self.slope is not None:
                self.slope.fill_(self.slope_init)

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or int(x.shape[-1]) != self.num_features:
            raise ValueError(f"SnapshotBatchNorm: an (N, {self.num_features}) or (L, N, {self.num_features}) tensor")
        batch_stats = self.training or not self.track_running_stats
        update = self.training and self.track_running_stats
        y = ops.batch_norm(x, self.weight, self.bias, self.running_mean if (update or not batch_stats) else None,
                           self.running_var if (update or not batch_stats) else None, training=batch_stats, momentum=self.momentum,
                           eps=self.eps, pre=self.pre, post=self.post, slope=self.slope)
        if update:
            self.num_batches_tracked += 1 if x.dim() == 2 else int(x.shape[0])
        return y

    def extra_repr(self):
        return (f"{self.num_features}, eps={self.eps}, momentum={self.momentum}, affine={self.affine}, "
                f"track_running_stats={self.track_running_stats}, pre={self.pre!r}, post={self.post!r}")


class SnapshotGINEncoder(torch.nn.Module):
    """scripts/graph_shared.py's GConv for all views of a call at once: per layer SnapshotGINConv(Linear-ReLU-Linear), then the
    fused SnapshotBatchNorm(hidden_dim, pre="relu") -- conv -> F.relu -> BatchNorm1d, every view with its own statistics --, then
    the readout of the layer's output.  forward(x, snapshots) takes x (n, input_dim), shared by the views, or (L, n, input_dim), and
    a `Snapshots` or its `.plan()` (anything with `.aggregate(x)` and `.readout(z)`); it returns the node embeddings
    (L, n, hidden_dim * num_layers) and the graph embeddings (L, G, hidden_dim * num_layers), the layers' outputs side by side as
    GConv concatenates them.  So the graph-level step is one (L, n, F) pipeline from the features to both embeddings, without a
    Python loop over the views.  (GConv's `project` head belongs to the contrast model around it and is not part of this.)
    `dense="device"` makes every layer's MLP a SnapshotMLP (ops.linear_act); the default leaves the Linears to torch."""

    def __init__(self, input_dim: int, hidden_dim: int, num_layers: int, dense: str = "torch"):
        super().__init__()
        dense = _dense_arg(dense)
        if num_layers < 1:
            raise ValueError("num_layers: at least one")
        self.layers = torch.nn.ModuleList()
        self.batch_norms = torch.nn.ModuleList()
        for i in range(num_layers):
            d = input_dim if i == 0 else hidden_dim
            self.layers.append(SnapshotGINConv(_gin_mlp(d, hidden_dim, dense)))
            self.batch_norms.append(SnapshotBatchNorm(hidden_dim, pre="relu"))

    def forward(self, x, snapshots):
        z, zs = x, []
        for conv, bn in zip(self.layers, self.batch_norms):
            z = bn(conv(z, snapshots))
            zs.append(z)
        gs = [snapshots.readout(z) for z in zs]
        return torch.cat(zs, dim=-1), torch.cat(gs, dim=-1)


class SnapshotActDropout(torch.nn.Module):
    """activation -> dropout behind a layer, for all views of a call at once: forward(x, bias=None) = ops.bias_act_dropout on an
    (L, N, F) tensor (or one (N, F) view) -- `conv -> PReLU -> F.dropout(p)` of scripts/graph_shared_g2l.py's GConv and
    `GCNConv -> PReLU` of scripts/node_shared.py in one pass, the layer's bias added on the way where it is handed over.  `act` is
    "none", "relu" or "prelu"; with "prelu" the slope is the parameter `weight` (`num_parameters` values, 0.25 at reset), as
    torch.nn.PReLU names it, so a state dict moves across.  `.eval()` switches the dropout off.  Every training forward draws a
    fresh seed from torch's generator unless an integer `seed` is given, which fixes the mask."""

    def __init__(self, act: str = "prelu", p: float = 0.0, num_parameters: int = 1, seed: Optional[int] = None):
        super().__init__()
        if act not in ops.ROW_ACT:
            raise ValueError(f"act: one of {sorted(ops.ROW_ACT)}")
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 <= p < 1.0):
            raise ValueError(f"p: a number in [0, 1), got {p!r}")
        self.act, self.p, self.num_parameters, self.seed = act, float(p), int(num_parameters), seed
        if act == "prelu":
            self.weight = torch.nn.Parameter(torch.empty(self.num_parameters))
        else:
            self.register_parameter("weight", None)
        self.reset_parameters()

    def reset_parameters(self):
        if self.weight is not None:
            with torch.no_grad():
                self.weight.fill_(0.25)

    def forward(self, x, bias=None):
        return ops.bias_act_dropout(x, bias, act=self.act, slope=self.weight, p=self.p, training=self.training, seed=self.seed)

    def extra_repr(self):
        return f"act={self.act!r}, p={self.p}, num_parameters={self.num_parameters}, seed={self.seed}"


class SnapshotLayerNorm(torch.nn.Module):
    """LayerNorm over the last dimension for all views of a call at once, with the activation and the dropout behind it fused in:
    forward(x) = ops.layer_norm on an (L, N, F) tensor (or one (N, F) view) -- the "layer" branch of the reference's Normalize, and
    with post="prelu" and p the `Normalize -> PReLU -> Dropout` of its projection head and predictor in one pass.  It restates
    torch.nn.LayerNorm's published semantics for one normalised dimension -- parameter names `weight` and `bias`, ones and zeros at
    reset, biased variance --, so a state dict moves across; with post="prelu" the module also carries the slope as the parameter
    `slope` (one value, 0.25 at reset).  `.eval()` switches the dropout off; an integer `seed` fixes the mask."""

    def __init__(self, num_features: int, eps: float = 1e-5, elementwise_affine: bool = True, post: str = "none", p: float = 0.0,
                 seed: Optional[int] = None):
        super().__init__()
        if post not in ops.ROW_ACT:
            raise ValueError(f"post: one of {sorted(ops.ROW_ACT)}")
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 <= p < 1.0):
            raise ValueError(f"p: a number in [0, 1), got {p!r}")
        self.num_features, self.eps, self.elementwise_affine = int(num_features), eps, bool(elementwise_affine)
        self.post, self.p, self.seed = post, float(p), seed
        if self.elementwise_affine:
            self.weight = torch.nn.Parameter(torch.empty(self.num_features))
            self.bias = torch.nn.Parameter(torch.empty(self.num_features))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        if post == "prelu":
            self.slope = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_parameter("slope", None)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            if self.elementwise_affine:
                self.weight.fill_(1.0)
                self.bias.zero_()
            if self.slope is not None:
                self.slope.fill_(0.25)

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or int(x.shape[-1]) != self.num_features:
            raise ValueError(f"SnapshotLayerNorm: an (N, {self.num_features}) or (L, N, {self.num_features}) tensor")
        return ops.layer_norm(x, self.weight, self.bias, eps=self.eps, post=self.post, slope=self.slope, p=self.p, training=self.training,
                              seed=self.seed)

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}, elementwise_affine={self.elementwise_affine}, post={self.post!r}, p={self.p}"


class SnapshotG2LEncoder(torch.nn.Module):
    """scripts/graph_shared_g2l.py's GConv for all views of a call at once: per layer SnapshotGINConv(Linear-ReLU-Linear) and the
    shared epilogue `activation` (one PReLU slope for all layers, as GConv's, with the dropout fused in); behind the stack
    `batch_norm`, a SnapshotBatchNorm or SnapshotLayerNorm as `encoder_norm` says ("batch", "layer" or "none"); then the projection
    head Linear -> norm(post="prelu") -> dropout.  With "layer" the head's PReLU and dropout are part of the layer-norm call; behind
    a batch norm, whose call is as it was, the dropout is an epilogue call of its own (`head_dropout`).  forward(x, snapshots) takes
    x (n, input_dim), shared by the views, or (L, n, input_dim), and a `Snapshots` or its `.plan()`; it returns (z, projection),
    both (L, n, hidden_dim).  An integer `seed` fixes every dropout mask (call c of a forward uses seed + 1000 c).
    `dense="device"` makes every layer's MLP a SnapshotMLP and the head's Linear a SnapshotLinear (ops.linear_act); the
    default leaves them to torch."""

    def __init__(self, input_dim: int, hidden_dim: int, num_layers: int, dropout: float = 0.2, encoder_norm: str = "batch",
                 projector_norm: str = "batch", seed: Optional[int] = None, dense: str = "torch"):
        super().__init__()
        dense = _dense_arg(dense)
        if num_layers < 1:
            raise ValueError("num_layers: at least one")
        for norm in (encoder_norm, projector_norm):
            if norm not in ("batch", "layer", "none"):
                raise ValueError('encoder_norm, projector_norm: "batch", "layer" or "none"')
        sub = (lambda c: None) if seed is None else (lambda c: int(seed) + 1000 * c)
        self.layers = torch.nn.ModuleList()
        for i in range(num_layers):
            d = input_dim if i == 0 else hidden_dim
            self.layers.append(SnapshotGINConv(_gin_mlp(d, hidden_dim, dense)))
        self.activation = SnapshotActDropout("prelu", dropout, seed=sub(0))
        self.layer_seeds = None if seed is None else [int(seed) + 1000 * (2 + i) for i in range(num_layers)]
        if encoder_norm == "batch":
            self.batch_norm = SnapshotBatchNorm(hidden_dim)
        elif encoder_norm == "layer":
            self.batch_norm = SnapshotLayerNorm(hidden_dim)
        else:
            self.batch_norm = torch.nn.Identity()
        self.head_linear = SnapshotLinear(hidden_dim, hidden_dim) if dense == "device" else torch.nn.Linear(hidden_dim, hidden_dim)
        if projector_norm == "batch":
            self.head_norm = SnapshotBatchNorm(hidden_dim, post="prelu")
            self.head_dropout = SnapshotActDropout("none", dropout, seed=sub(1))
        elif projector_norm == "layer":
            self.head_norm = SnapshotLayerNorm(hidden_dim, post="prelu", p=dropout, seed=sub(1))
            self.head_dropout = torch.nn.Identity()
        else:
            self.head_norm = SnapshotActDropout("prelu", dropout, seed=sub(1))
            self.head_dropout = torch.nn.Identity()

    def forward(self, x, snapshots):
        z = x
        for i, conv in enumerate(self.layers):
            z = conv(z, snapshots)
            act = self.activation
            z = ops.bias_act_dropout(z, None, act=act.act, slope=act.weight, p=act.p, training=self.training,
                                     seed=None if self.layer_seeds is None else self.layer_seeds[i])
        z = self.batch_norm(z)
        return z, self.head_dropout(self.head_norm(self.head_linear(z)))


def update_target(target: torch.nn.Module, online: torch.nn.Module, momentum: float) -> None:
    """The bootstrap's moving average, p_target = momentum * p_target + (1 - momentum) * p_online over the parameters in order
    (scripts/graph_shared_g2l.py: Encoder.update_target_encoder), in two torch._foreach calls.  A convenience, not a kernel."""
    tp, op = [p.data for p in target.parameters()], [p.data for p in online.parameters()]
    if len(tp) != len(op):
        raise ValueError("update_target: the two modules differ in their parameters")
    with torch.no_grad():
        torch._foreach_mul_(tp, float(momentum))
        torch._foreach_add_(tp, op, alpha=1.0 - float(momentum))


class NodeContrast(torch.nn.Module):
    """The contrastive loss of the node-level training step: forward(h1, h2) = 0.5 * (info_nce(h1, h2) + info_nce(h2, h1)), what
    DualBranchContrast(InfoNCEBatched(tau, batch_size), mode="L2L") of scripts/node_shared.py computes, by two ops.info_nce calls
    (no N x N matrix, fixed summation order, memory O(N F)).  h1, h2 are (N, F) float32 embeddings of two views; given one
    (L, N, F) tensor of L >= 2 views, as SnapshotGCNConv returns it, forward(h) contrasts view 0 with view 1.  `positive="raw"`
    (the default) restates the reference's InfoNCEBatched, whose positive term s_ii is not divided by tau; "scaled" is GCL's
    InfoNCE.  The loss is a 0-dim float64 tensor; gradients reach both views.  `pair=True` computes the same loss by one
    ops.info_nce_pair call -- both directions from one pass over the similarities, half the products -- whose value differs from the
    two calls' in the order of the sums alone.  `intraview_negs` is DualBranchContrast's switch: True adds every other row of the
    anchor's own view to each denominator ("masked": what the sampler gives GCL's InfoNCE, the loss of GRACE); "all" also counts
    the row itself, which is what InfoNCEBatched computes under that sampler, since it never reads the masks; False (the default)
    leaves the loss as it was.  It works with either setting of `pair`."""

    INTRAVIEW = {False: "none", True: "masked", "none": "none", "masked": "masked", "all": "all"}

    def __init__(self, tau: float = 0.4, positive: str = "raw", pair: bool = False, intraview_negs=False):
        super().__init__()
        if not isinstance(intraview_negs, (bool, str)) or intraview_negs not in self.INTRAVIEW:
            raise ValueError(f'intraview_negs: False, True ("masked") or "all", got {intraview_negs!r}')
        self.tau, self.positive, self.pair = tau, positive, bool(pair)
        self.intraview = self.INTRAVIEW[intraview_negs]

    def forward(self, h1, h2=None):
        if h2 is None:
            if not isinstance(h1, torch.Tensor) or h1.dim() != 3 or h1.shape[0] < 2:
                raise ValueError("NodeContrast: two (N, F) embeddings, or one (L, N, F) tensor of L >= 2 views")
            h1, h2 = h1[0], h1[1]
        if self.pair:
            return ops.info_nce_pair(h1, h2, tau=self.tau, positive=self.positive, intraview=self.intraview)
        l1 = ops.info_nce(h1, h2, tau=self.tau, positive=self.positive, intraview=self.intraview)
        l2 = ops.info_nce(h2, h1, tau=self.tau, positive=self.positive, intraview=self.intraview)
        return 0.5 * (l1 + l2)


class CCAContrast(torch.nn.Module):
    """The loss of CCA-SSG/main.py: forward(h1, h2) = ops.cca_loss(h1, h2, lambd), the standardisation of CCA-SSG/model.py included
    -- h1, h2 are the encoder's outputs, not the standardised z.  h1, h2 are (N, F) float32 embeddings of two views; given one
    (L, N, F) tensor of L >= 2 views, as SnapshotGCNConv returns it, forward(h) takes view 0 against view 1.  The loss is a 0-dim
    float64 tensor; gradients reach both views."""

    def __init__(self, lambd: float = 1e-3):
        super().__init__()
        self.lambd = lambd

    def forward(self, h1, h2=None):
        if h2 is None:
            if not isinstance(h1, torch.Tensor) or h1.dim() != 3 or h1.shape[0] < 2:
                raise ValueError("CCAContrast: two (N, F) embeddings, or one (L, N, F) tensor of L >= 2 views")
            h1, h2 = h1[0], h1[1]
        return ops.cca_loss(h1, h2, lambd=self.lambd)


class BarlowTwinsContrast(torch.nn.Module):
    """PyGCL's WithinEmbedContrast(L.BarlowTwins()), the G-BT baseline: forward(h1, h2) = ops.barlow_twins_loss(h1, h2, lambd, eps),
    the standardisation included.  h1, h2 are (N, F) float32 embeddings of two views; given one (L, N, F) tensor of L >= 2 views, as
    SnapshotGCNConv returns it, forward(h) takes view 0 against view 1.  lambd=None means 1 / F.  WithinEmbedContrast averages
    loss(h1, h2) and loss(h2, h1); the cross-correlation of the swapped call is the transpose of the first's, and the loss sums the
    same diagonal and the same off-diagonal squares, so the two are one value and this module makes ONE call.  The loss is a 0-dim
    float64 tensor; gradients reach both views."""

    def __init__(self, lambd: Optional[float] = None, eps: float = 1e-15):
        super().__init__()
        self.lambd = lambd
        self.eps = eps

    def forward(self, h1, h2=None):
        if h2 is None:
            if not isinstance(h1, torch.Tensor) or h1.dim() != 3 or h1.shape[0] < 2:
                raise ValueError("BarlowTwinsContrast: two (N, F) embeddings, or one (L, N, F) tensor of L >= 2 views")
            h1, h2 = h1[0], h1[1]
        return ops.barlow_twins_loss(h1, h2, lambd=self.lambd, eps=self.eps)


def _view_pair(x, y, what: str, name: str):
    """(x, y), or the first two views of one (L, rows, F) tensor of L >= 2 views given as x."""
    if y is None:
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[0] < 2:
            raise ValueError(f"{name}: two (rows, F) tensors for {what}, or one (L, rows, F) tensor of L >= 2 views")
        return x[0], x[1]
    return x, y


class G2LContrast(torch.nn.Module):
    """The graph-to-local contrastive loss of scripts/node_dedicated.py: forward(h1, h2, g1, g2, h3, h4, node_ptr) =
    0.5 * (g2l_jsd(h2, g1, neg=h4) + g2l_jsd(h1, g2, neg=h3)), the single-graph and the multi-graph branch of the reference's
    DualBranchContrast(JSD(), mode="G2L") (scripts/node_shared.py: the text of the branches; the sampler restates PyGCL's published
    CrossScaleSampler, which is not installed here), by two ops.g2l_jsd calls.  h1, h2 are (N, F) float32 node embeddings of two
    views, g1, g2 (G, F) their graph summaries, h3, h4 the embeddings of the corrupted input (adapters.corrupt), required exactly
    when there is one graph; node_ptr the batch's table (None: one graph).  Given (L, N, F) / (L, G, F) tensors of L >= 2 views in
    place of a pair (h2, g2, h4 = None), views 0 and 1 are taken.  The loss is a 0-dim float64 tensor; gradients reach h, g and the
    corrupted embeddings."""

    def forward(self, h1, h2=None, g1=None, g2=None, h3=None, h4=None, node_ptr=None):
        h1, h2 = _view_pair(h1, h2, "h1, h2", "G2LContrast")
        g1, g2 = _view_pair(g1, g2, "g1, g2", "G2LContrast")
        if h3 is not None or h4 is not None:
            h3, h4 = _view_pair(h3, h4, "h3, h4", "G2LContrast")
        l1 = ops.g2l_jsd(h2, g1, node_ptr=node_ptr, neg=h4)
        l2 = ops.g2l_jsd(h1, g2, node_ptr=node_ptr, neg=h3)
        return 0.5 * (l1 + l2)


class BootstrapG2L(torch.nn.Module):
    """The graph-to-local bootstrap loss of scripts/graph_shared_g2l.py: forward(h1_pred, h2_pred, g1_target, g2_target, node_ptr) =
    0.5 * (g2l_bootstrap(h2_pred, g1_target) + g2l_bootstrap(h1_pred, g2_target)), what BootstrapContrast(BootstrapLatent(),
    mode="G2L") computes (restated from PyGCL as published; it is not installed here), by two ops.g2l_bootstrap calls.  The targets
    are detached, as the script does.  Given (L, N, F) / (L, G, F) tensors of L >= 2 views in place of a pair, views 0 and 1 are
    taken.  The loss is a 0-dim float64 tensor; gradients reach the predictions alone."""

    def forward(self, h1_pred, h2_pred=None, g1_target=None, g2_target=None, node_ptr=None):
        h1_pred, h2_pred = _view_pair(h1_pred, h2_pred, "h1_pred, h2_pred", "BootstrapG2L")
        g1_target, g2_target = _view_pair(g1_target, g2_target, "g1_target, g2_target", "BootstrapG2L")
        l1 = ops.g2l_bootstrap(h2_pred, g1_target.detach(), node_ptr=node_ptr)
        l2 = ops.g2l_bootstrap(h1_pred, g2_target.detach(), node_ptr=node_ptr)
        return 0.5 * (l1 + l2)


def corrupt(x, generator=None):
    """scripts/node_dedicated.py's `corruption`: the rows of x in a random order, x[randperm(N)] (from `generator`, on x's device).
    Plain torch."""
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise ValueError("corrupt: x is a tensor with rows")
    return x[torch.randperm(x.size(0), device=x.device, generator=generator)]


def drop_feature(x, p: float, views: int = 1, generator=None):
    """CCA-SSG/aug.py's drop_feature (A.FeatureMasking of the PyGCL scripts) for `views` views at once: per view, F uniforms are
    drawn (from `generator`, on x's device) and the columns with u < p are set to zero.  x is (N, F); returns (views, N, F), which
    SnapshotGCNConv takes as its per-view x.  Plain torch.  For features that stay the same over a run, ops.feature_plan(x) with the
    masks of ops.feature_masks gives the same products without the `views` dense copies."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("drop_feature: x is a (N, F) tensor")
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"drop_feature: p in [0, 1], got {p!r}")
    if isinstance(views, bool) or not isinstance(views, int) or views < 1:
        raise ValueError(f"drop_feature: views >= 1, got {views!r}")
    out = x.unsqueeze(0).repeat(views, 1, 1)
    for v in range(views):
        mask = torch.empty((x.size(1),), dtype=torch.float32, device=x.device).uniform_(0, 1, generator=generator) < p
        out[v][:, mask] = 0
    return out


def graph_plan(g, fill_value: float = 1.0, directions: str = "both"):
    """The propagation plan of the input graph itself (ops.edge_plan): `g` is an (x, edge_index, edge_weights) triple or a Graph
    (anything with `.unfold()`); weighted iff edge_weights is given; the loops cover x.shape[0] ids (what GCNConv uses), or
    edge_index.max() + 1 without x.  SnapshotGCNConv.forward(x, graph_plan(g)) is then the encoder's z of the un-augmented graph,
    with the normalisation, the summation order and the bits of the views' plans."""
    x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
    return ops.edge_plan(edge_index, edge_weights, int(x.shape[0]) if x is not None else None, add_self_loops=True, fill_value=fill_value,
                         normalize=True, directions=directions)


class rLap:
    """PyGCL-style augmentor: `aug(x, edge_index, edge_weight)` or `aug.augment(g)` with g.unfold().

    Reference (scripts/augmentor_benchmarks.py:68-96): num_remove = int(frac * num_nodes);
    the returned graph drops the Schur-complement weights (`edge_weights=None`, :96) unless
    keep_weights=True.
    """

    def __init__(self, frac: float, o_v: str = "random", o_n: str = "asc", keep_weights: bool = False, seed: Optional[int] = None,
                 num_nodes_from_x: bool = False, symmetrize: bool = False, gcn_norm: bool = False, fill_value: float = 1.0):
        self.frac = frac
        self.o_v = o_v
        self.o_n = o_n
        self.keep_weights = keep_weights
        self.seed = seed
        self.num_nodes_from_x = num_nodes_from_x
        self.symmetrize = symmetrize      # True: one-directional input is made undirected inside the op (fused to_undirected)
        self.gcn_norm, self.fill_value = gcn_norm, fill_value   # True: self loops and GCN coefficients (_gcn_graphs)

    def augment(self, g):
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        sc, num_nodes = _schur(edge_index, edge_weights, x, self.frac, self.o_v, self.o_n, self.seed, self.num_nodes_from_x, self.symmetrize)
        self.num_remove = int(self.frac * num_nodes)
        if self.gcn_norm:
            return _gcn_graphs(x, sc, [0, int(sc.shape[0])], num_nodes, self.keep_weights, self.fill_value)[0]
        sampled_edge_index = sc[:, :2].long().t().contiguous()          # stays on the device
        w = sc[:, 2].contiguous() if self.keep_weights else None
        try:  # PyGCL present: return its Graph type
            import GCL.augmentors as A  # type: ignore
            return A.Graph(x=x, edge_index=sampled_edge_index, edge_weights=w)
        except Exception:
            return Graph(x, sampled_edge_index, w)

    def snapshots(self, g) -> Snapshots:
        """The one elimination call of `augment` as a `Snapshots` holder (one layer)."""
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        sc, num_nodes = _schur(edge_index, edge_weights, x, self.frac, self.o_v, self.o_n, self.seed, self.num_nodes_from_x, self.symmetrize)
        self.num_remove = int(self.frac * num_nodes)
        return _snapshots_of(x, sc, [0, int(sc.shape[0])], num_nodes, self.keep_weights, self.fill_value)

    def __call__(self, x, edge_index, edge_weight=None):
        return self.augment(Graph(x, edge_index, edge_weight))


def _as_graph(x, edge_index, w):
    try:  # PyGCL present: return its Graph type
        import GCL.augmentors as A  # type: ignore
        return A.Graph(x=x, edge_index=edge_index, edge_weights=w)
    except Exception:
        return Graph(x, edge_index, w)


def _gcn_graphs(x, sc, ptr, num_nodes, keep_weights, fill_value):
    """The snapshots of one call as GCNConv(..., normalize=False) takes them, from ONE ops.snapshot_gcn_norm call: for every segment
    Graph(x, edge_index, edge_weights) with the self loops in edge_index (int64) and the float32 coefficients deg^-1/2 w deg^-1/2 as
    edge_weights -- weighted iff keep_weights.  The loops cover x.shape[0] nodes when x is given (what GCNConv uses), else the call's
    num_nodes.  Segment s is a slice of the call's one (2, M) tensor: nothing is copied."""
    n = int(x.shape[0]) if x is not None else int(num_nodes)
    ei, w, eptr = ops.snapshot_gcn_norm(sc, ptr, n, weighted=keep_weights, fill_value=fill_value)
    e = eptr.tolist()
    return [_as_graph(x, ei[:, e[i]:e[i + 1]], w[e[i]:e[i + 1]]) for i in range(len(e) - 1)]


class rLapViews:
    """K views of a graph from ONE call of ops.approximate_cholesky_views (setup once, K eliminations side by side).

    View k removes int(fracs[k] * num_nodes) vertices, num_nodes = edge_index.max() + 1 (scripts/augmentor_benchmarks.py:77-78).
    `.augment(g)` returns the list of K graphs.  `.augmentors()` returns K PyGCL-style callables that fit the `(aug1, aug2)` tuple
    of the training scripts unchanged: the first one called on an input makes the one call, the others then take their views.
    """

    def __init__(self, fracs=(0.5, 0.5), o_v: str = "random", o_n: str = "asc", keep_weights: bool = False, seed: Optional[int] = None,
                 mode: str = "exact", gcn_norm: bool = False, fill_value: float = 1.0):
        self.fracs = tuple(float(f) for f in fracs)
        assert len(self.fracs) >= 1
        self.o_v, self.o_n, self.keep_weights, self.seed, self.mode = o_v, o_n, keep_weights, seed, mode
        self.gcn_norm, self.fill_value = gcn_norm, fill_value   # True: self loops and GCN coefficients (_gcn_graphs)
        self._pending = None   # (input key, list of K graphs, list of views not yet handed out)

    def _call(self, g):
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        num_nodes = int(edge_index.max().item()) + 1 if edge_index.numel() else 0
        self.num_remove = [int(f * num_nodes) for f in self.fracs]
        sc, ptr = ops.approximate_cholesky_views(edge_index, edge_weights, num_nodes, self.num_remove, self.o_v, self.o_n,
                                                 seed=self.seed, return_device="same", mode=self.mode)
        return x, sc, ptr, num_nodes

    def snapshots(self, g, node_ptr=None) -> Snapshots:
        """The one elimination call of `augment` as a `Snapshots` holder: layer k is view k.

        `node_ptr` ([G+1] offsets, node_ptr_of(batch)): g is a batch of G graphs, graph j owning the ids [node_ptr[j],
        node_ptr[j+1]).  The one call then eliminates every graph on its own (ops.approximate_cholesky_views(node_ptr=)): view k
        removes int(fracs[k] * n_j) vertices of graph j, n_j its node count -- a (K, G) table, kept as `num_remove` -- and the holder
        keeps `node_ptr`, so `.readout(z)` pools per graph.  This DIFFERS from scripts/graph_shared.py, which hands the disjoint
        union of the batch to the augmentor as ONE graph with one global count int(frac * num_nodes): there a graph of the batch
        may lose any share of its vertices, here each loses its own fraction."""
        if node_ptr is None:
            x, sc, ptr, num_nodes = self._call(g)
            return _snapshots_of(x, sc, ptr, num_nodes, self.keep_weights, self.fill_value)
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        np_, n, self.num_remove = _batch_tables(node_ptr, x, self.fracs)
        sc, ptr = ops.approximate_cholesky_views(edge_index, edge_weights, n, self.num_remove, self.o_v, self.o_n, node_ptr=np_,
                                                 seed=self.seed, return_device="same", mode=self.mode)
        return Snapshots(sc, ptr, n, np_, self.keep_weights, self.fill_value)

    def augment(self, g):
        x, sc, ptr, num_nodes = self._call(g)
        if self.gcn_norm:
            return _gcn_graphs(x, sc, ptr, num_nodes, self.keep_weights, self.fill_value)
        out = []
        for k in range(len(self.fracs)):
            part = sc[int(ptr[k]):int(ptr[k + 1])]
            ei = part[:, :2].long().t().contiguous()
            out.append(_as_graph(x, ei, part[:, 2].contiguous() if self.keep_weights else None))
        return out

    @staticmethod
    def _key(edge_index):
        return (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), str(edge_index.device))

    def _view(self, k, g):
        """View k of input g: taken from the pending call when that call was made on this very input and view k has not been
        handed out yet; otherwise a fresh call (whose other views are then pending)."""
        edge_index = g.unfold()[1] if hasattr(g, "unfold") else g[1]
        key = self._key(edge_index)
        p = self._pending
        if p is None or p[0] != key or k not in p[2]:
            graphs = self.augment(g)
            # (the input is held while views are pending: its memory cannot be reused by another tensor with the same key)
            p = self._pending = (key, graphs, set(range(len(graphs))), edge_index)
        p[2].discard(k)
        res = p[1][k]
        if not p[2]:
            self._pending = None
        return res

    def augmentors(self):
        return [_ViewAugmentor(self, k) for k in range(len(self.fracs))]


class rLapDepths:
    """The graph at K removed fractions from ONE call of ops.approximate_cholesky_depths (one elimination, a snapshot at every
    depth).  Depth k removes int(fracs[k] * num_nodes) vertices, num_nodes = edge_index.max() + 1, as rLap does; the fractions
    are taken in the order given and must not decrease.  `.augment(g)` returns the K graphs; node ids stay in the input's space,
    so no relabel is needed between depths.  Graph k equals rLap(fracs[k], ...).augment(g) with the same seed.

    `views=R` (an int): R independent runs of the sweep (the `num_runs` loop of scripts/rlap_vc_spectral.py) from the same ONE
    call, as R views side by side; `.augment(g)` then returns R lists of K graphs, list r being run r (view r of
    ops.approximate_cholesky_depths(..., views=R)).  `views=None` keeps the flat list of K graphs.
    """

    def __init__(self, fracs=(0.1, 0.2, 0.3), o_v: str = "random", o_n: str = "asc", keep_weights: bool = False, seed: Optional[int] = None,
                 mode: str = "exact", views: Optional[int] = None, gcn_norm: bool = False, fill_value: float = 1.0):
        self.fracs = tuple(float(f) for f in fracs)
        assert len(self.fracs) >= 1
        assert views is None or (int(views) == views and views >= 1), "views: None or a positive int"
        self.o_v, self.o_n, self.keep_weights, self.seed, self.mode, self.views = o_v, o_n, keep_weights, seed, mode, views
        self.gcn_norm, self.fill_value = gcn_norm, fill_value   # True: self loops and GCN coefficients (_gcn_graphs)

    def _snapshots(self, g):
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        num_nodes = int(edge_index.max().item()) + 1 if edge_index.numel() else 0
        self.num_remove = [int(f * num_nodes) for f in self.fracs]
        extra = {} if self.views is None else {"views": int(self.views)}
        sc, ptr = ops.approximate_cholesky_depths(edge_index, edge_weights, num_nodes, self.num_remove, self.o_v, self.o_n,
                                                  seed=self.seed, return_device="same", mode=self.mode, **extra)
        return x, sc, ptr, num_nodes

    def snapshots(self, g, node_ptr=None) -> Snapshots:
        """The one elimination call of `augment` as a `Snapshots` holder: layer k * R + r is depth k of run r (depth-major, then
        view, as the rows are).

        `node_ptr` ([G+1] offsets, node_ptr_of(batch)): g is a batch of G graphs and the one call eliminates every graph on its
        own (ops.approximate_cholesky_depths(node_ptr=)): depth k removes int(fracs[k] * n_j) vertices of graph j, n_j its node
        count -- a (D, R, G) table, kept as `num_remove` -- and the holder keeps `node_ptr`.  This DIFFERS from
        scripts/graph_shared.py, which eliminates the disjoint union of the batch as ONE graph with one global count
        int(frac * num_nodes)."""
        if node_ptr is None:
            x, sc, ptr, num_nodes = self._snapshots(g)
            return _snapshots_of(x, sc, ptr, num_nodes, self.keep_weights, self.fill_value)
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        np_, n, table = _batch_tables(node_ptr, x, self.fracs)
        R = 1 if self.views is None else int(self.views)
        self.num_remove = [[row] * R for row in table]
        sc, ptr = ops.approximate_cholesky_depths(edge_index, edge_weights, n, self.num_remove, self.o_v, self.o_n, node_ptr=np_, views=R,
                                                  seed=self.seed, return_device="same", mode=self.mode)
        return Snapshots(sc, ptr, n, np_, self.keep_weights, self.fill_value)

    def stats(self, g, weighted: bool = False, tol: float = 1e-10, max_iter: int = 1000):
        """The three lists scripts/rlap_vc_spectral.py records per snapshot (get_rlap_sc_stats: max_sv, num_unique_nodes, num_edges)
        for every run and depth of ONE call, computed on the device by ops.snapshot_stats: a dict of (runs, depths) tensors
        `max_sv` (float64: the largest eigenvalue of the unweighted adjacency, or with `weighted` of the Schur-complement weights),
        `node_count` and `edge_count` (int64: distinct ids and directed rows), plus `converged` (bool).  runs = views (1 with
        views=None): row r is run r, column k depth fracs[k] -- the layout plot_sv_trend / plot_edge_count_trend average over."""
        _, sc, ptr, num_nodes = self._snapshots(g)
        st = ops.snapshot_stats(sc, ptr, num_nodes, weighted=weighted, tol=tol, max_iter=max_iter)
        D, R = len(self.fracs), 1 if self.views is None else int(self.views)

        def grid(t):   # (snapshots are depth-major, then view)
            return t.reshape(D, R).t().contiguous()
        return {"max_sv": grid(st["lambda_max"]), "node_count": grid(st["nodes"]), "edge_count": grid(st["rows"]),
                "converged": grid(st["converged"])}

    def _diffused(self, sc, ptr, num_nodes, alpha, eps, tol, kind, order):
        """(out, pptr) of the one diffusion call over all snapshots: ops.snapshot_ppr, or with kind="markov" ops.snapshot_markov."""
        if kind == "ppr":
            return ops.snapshot_ppr(sc, ptr, num_nodes, alpha=alpha, eps=eps, tol=tol)
        if kind == "markov":
            return ops.snapshot_markov(sc, ptr, num_nodes, alpha=alpha, order=order, eps=eps)
        raise ValueError(f'kind: "ppr" or "markov", got {kind!r}')

    def diffuse(self, g, alpha: float = 0.2, eps: float = 1e-4, tol: float = 1e-10, kind: str = "ppr", order: int = 16):
        """rLapPPRDiffusion's graph (Schur-complement weights -> PPR diffusion, normalised) for every run and depth of ONE call: one
        depths call and one ops.snapshot_ppr call -- the fraction sweep of scripts/rlap_ppr_edge_plots.py from one elimination.
        kind="markov" takes the Markov diffusion of ops.snapshot_markov (its defaults: self loop, not normalised) with `order` in
        its place; `tol` is then unused.
        Returns the layout of `augment`: K graphs, or R lists of K with views=R; each is Graph(x, edge_index, edge_weights) with
        ids in the input's space, as rLapPPRDiffusion returns."""
        x, sc, ptr, num_nodes = self._snapshots(g)
        out, pptr = self._diffused(sc, ptr, num_nodes, alpha, eps, tol, kind, order)
        pp = pptr.cpu()

        def graph(i):
            part = out[int(pp[i]):int(pp[i + 1])]
            return Graph(x, part[:, :2].long().t().contiguous(), part[:, 2].contiguous())
        K = len(self.fracs)
        if self.views is None:
            return [graph(k) for k in range(K)]
        R = int(self.views)
        return [[graph(k * R + r) for k in range(K)] for r in range(R)]

    def diffuse_plan(self, g, alpha: float = 0.2, eps: float = 1e-4, tol: float = 1e-10, directions: str = "both", kind: str = "ppr",
                     order: int = 16):
        """One propagation plan over all diffused snapshots of `diffuse`: straight from the (out, pptr) of the one ops.snapshot_ppr
        (kind="markov": ops.snapshot_markov) call to ops.edge_list_plan(weighted=True) -- no slicing, no edge_index.  Layer i is
        snapshot i in pptr order (depth-major, then view, as the rows are); the loops cover x.shape[0] ids when x is given, with this
        augmentor's fill_value."""
        x, sc, ptr, num_nodes = self._snapshots(g)
        out, pptr = self._diffused(sc, ptr, num_nodes, alpha, eps, tol, kind, order)
        n = int(x.shape[0]) if x is not None else int(num_nodes)
        return ops.edge_list_plan(out, pptr, n, weighted=True, add_self_loops=True, fill_value=self.fill_value, normalize=True,
                                  directions=directions)

    def relabelled(self, g):
        """The compact graph of every run and depth and its id map -- torch.unique + subgraph(relabel_nodes=True) of every snapshot
        -- from ONE depths call and ONE ops.snapshot_subgraph call.  Returns the layout of `augment` with items
        (Graph(None, edge_index, edge_weights), ids): edge_index holds labels 0..len(ids)-1 and ids[label] is the input's id."""
        _, sc, ptr, num_nodes = self._snapshots(g)
        out, optr, ids, iptr = ops.snapshot_subgraph(sc, ptr, num_nodes, relabel=True)
        op, ip = optr.tolist(), iptr.tolist()

        def item(i):
            part = out[op[i]:op[i + 1]]
            return Graph(None, part[:, :2].long().t().contiguous(), part[:, 2].contiguous()), ids[ip[i]:ip[i + 1]]
        K = len(self.fracs)
        if self.views is None:
            return [item(k) for k in range(K)]
        R = int(self.views)
        return [[item(k * R + r) for k in range(K)] for r in range(R)]

    def batch_edge_counts(self, g, batch_size: int, generator=None, alpha: float = 0.2, eps: float = 1e-4):
        """The number scripts/rlap_ppr_edge_plots.py:61-76 plots, for every run and depth of ONE call: the diffusion of `diffuse`,
        its nodes without self loops (ops.snapshot_subgraph(remove_self_loops=True): remove_self_loops + unique), a random batch of
        up to `batch_size` of them (torch.randperm, seeded by `generator`, snapshot after snapshot in depth-major order) and the rows
        of the diffused graph among the batch (ops.snapshot_subgraph(nodes=, nodes_ptr=); as in the script the self loops count).
        Returns (counts, batches): counts a (runs, depths) int64 tensor, the layout of `stats`; batches the chosen node ids in
        the layout of `augment`."""
        _, sc, ptr, num_nodes = self._snapshots(g)
        out, pptr = ops.snapshot_ppr(sc, ptr, num_nodes, alpha=alpha, eps=eps)
        _, _, ids, iptr = ops.snapshot_subgraph(out, pptr, num_nodes, remove_self_loops=True)
        ip = iptr.tolist()
        gdev = generator.device if generator is not None else torch.device("cpu")
        chosen = []
        for s in range(len(ip) - 1):
            perm = torch.randperm(ip[s + 1] - ip[s], generator=generator, device=gdev)[:int(batch_size)]
            chosen.append(ids[ip[s]:ip[s + 1]][perm.to(ids.device)])
        nodes_ptr = [0]
        for c in chosen:
            nodes_ptr.append(nodes_ptr[-1] + int(c.numel()))
        _, optr, _, _ = ops.snapshot_subgraph(out, pptr, num_nodes, nodes=torch.cat(chosen), nodes_ptr=nodes_ptr)
        D, R = len(self.fracs), 1 if self.views is None else int(self.views)
        counts = (optr[1:] - optr[:-1]).reshape(D, R).t().contiguous()
        if self.views is None:
            return counts, chosen
        return counts, [[chosen[k * R + r] for k in range(D)] for r in range(R)]

    def augment(self, g):
        x, sc, ptr, num_nodes = self._snapshots(g)

        def graph(i):
            part = sc[int(ptr[i]):int(ptr[i + 1])]
            ei = part[:, :2].long().t().contiguous()
            return _as_graph(x, ei, part[:, 2].contiguous() if self.keep_weights else None)
        if self.gcn_norm:   # (one call for all snapshots; the same order)
            graph = _gcn_graphs(x, sc, ptr, num_nodes, self.keep_weights, self.fill_value).__getitem__
        K = len(self.fracs)
        if self.views is None:
            return [graph(k) for k in range(K)]
        R = int(self.views)
        return [[graph(k * R + r) for k in range(K)] for r in range(R)]   # (rows depth-major, then view)

    def __call__(self, x, edge_index, edge_weight=None):
        return self.augment(Graph(x, edge_index, edge_weight))


class rLapChain:
    """The chain of scripts/rlap_vc_spectral.py:14-58 (get_rlap_sc_stats): `batch_count` rounds, each an approximate_cholesky call on
    the relabelled, weighted result of the round before.  num_nodes_0 = edge_index.max() + 1 and every round removes
    t = int(batch_frac * num_nodes_0) vertices (the script's nodes_to_eliminate).  After a round the survivors that still have an
    edge are relabelled 0..k-1 by ONE ops.snapshot_subgraph(relabel=True) call on the device (no torch.unique), survivors without
    an edge drop out, num_nodes becomes k and the next round draws a fresh order: round k runs with `seed + k`.  This is not
    rLapDepths, whose depths are nested stops of one elimination in the input's id space.

    `perms` (o_v="random" only): an optional callable perms(k, num_nodes_k) returning round k's node_id vector, handed on as
    `perm=`; without it every round's order is drawn on the device from seed + k.  Per round the host reads one number, the node
    count the next call's arguments need.  A round whose result has no rows ends the chain: the remaining rounds are empty graphs.

    `.augment(g)` returns the batch_count graphs Graph(x, edge_index, edge_weights), ids mapped back into the input's space (the
    rounds' label -> id maps composed on the device) and the Schur-complement weights kept, as the next round uses them.
    """

    def __init__(self, batch_frac: float, batch_count: int, o_v: str = "random", o_n: str = "asc", seed: Optional[int] = None,
                 mode: str = "exact", perms=None):
        assert int(batch_count) == batch_count and batch_count >= 1, "batch_count: a positive int"
        assert perms is None or o_v == "random", "perms: only for o_v='random'"
        self.batch_frac, self.batch_count = float(batch_frac), int(batch_count)
        self.o_v, self.o_n, self.seed, self.mode, self.perms = o_v, o_n, seed, mode, perms

    def _rounds(self, g):
        """[(relabelled rows (m_k, 3), ids_k -> input ids, num_nodes_k of the round's result)] for every round."""
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        n = int(edge_index.max().item()) + 1 if edge_index.numel() else 0
        self.num_remove = int(self.batch_frac * n)
        seed = int(torch.randint(0, 2**62, (1,)).item()) if self.seed is None else int(self.seed)
        ei, w, back, rounds = edge_index, edge_weights, None, []
        if n == 0:
            rounds.append((torch.zeros((0, 3), dtype=torch.float64, device=edge_index.device),
                           torch.zeros(0, dtype=torch.int64, device=edge_index.device), 0))
        for k in range(len(rounds), self.batch_count):
            if rounds and rounds[-1][0].shape[0] == 0:      # nothing left to eliminate from: num_nodes would be 0
                rounds.append(rounds[-1])
                continue
            perm = None
            if self.perms is not None:
                perm = torch.as_tensor(self.perms(k, n), dtype=torch.int64)
            sc = ops.approximate_cholesky(ei, w, n, self.num_remove, self.o_v, self.o_n, perm=perm, seed=seed + k,
                                          return_device="same", mode=self.mode)
            out, _, ids, _ = ops.snapshot_subgraph(sc, [0, int(sc.shape[0])], n, relabel=True)
            back = ids if back is None else back[ids]
            n = int(ids.numel())
            rounds.append((out, back, n))
            ei, w = out[:, :2].long().t().contiguous(), out[:, 2].contiguous()
        return x, rounds

    def augment(self, g):
        x, rounds = self._rounds(g)
        return [_as_graph(x, back[out[:, :2].long()].t().contiguous(), out[:, 2].contiguous()) for out, back, _ in rounds]

    def stats(self, g, weighted: bool = False, tol: float = 1e-10, max_iter: int = 1000):
        """max_sv, node_count, edge_count (and converged) of every round through ONE ops.snapshot_stats call on the rounds'
        relabelled results: (1, batch_count) tensors, the layout of rLapDepths.stats with one run."""
        _, rounds = self._rounds(g)
        ptr = [0]
        for out, _, _ in rounds:
            ptr.append(ptr[-1] + int(out.shape[0]))
        st = ops.snapshot_stats(torch.cat([out for out, _, _ in rounds]), ptr, max(max(n for _, _, n in rounds), 1),
                                weighted=weighted, tol=tol, max_iter=max_iter)
        return {"max_sv": st["lambda_max"][None], "node_count": st["nodes"][None], "edge_count": st["rows"][None],
                "converged": st["converged"][None]}

    def __call__(self, x, edge_index, edge_weight=None):
        return self.augment(Graph(x, edge_index, edge_weight))


class _ViewAugmentor:
    """One sibling of rLapViews.augmentors(): `aug(x, edge_index, edge_weight)` or `aug.augment(g)`."""

    def __init__(self, parent, k: int):
        self.parent, self.k = parent, k

    def augment(self, g):
        return self.parent._view(self.k, g)

    def __call__(self, x, edge_index, edge_weight=None):
        return self.augment(Graph(x, edge_index, edge_weight))


class _EdgeDrop:
    """What the four edge-dropping augmentors share: one ops.drop_edges call, one view.  `seed=None` (the default) draws a fresh
    seed from torch's RNG at every call, as adapters.rLap does, so two augmentors built with the same arguments -- the reference's
    `(aug1, aug2)` -- and two calls of one give independent views; an integer seed makes every call return the same view.
    `last_seed` is the seed of the latest call.  num_nodes is edge_index.max() + 1, as the reference's lines compute it: one
    reduction and read-back in front of the call."""
    scheme = "uniform"

    def __init__(self, p: float, threshold: float = 0.7, seed: Optional[int] = None, aggr: str = "sink"):
        self.p, self.threshold, self.seed, self.aggr = p, threshold, seed, aggr
        self.last_seed = None

    def augment(self, g):
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        self.last_seed = ops._seed_from(self.seed)
        rows, _ = ops.drop_edges(edge_index, edge_weights, None, self.p, self.scheme, self.threshold, self.last_seed, self.aggr)
        return _as_graph(x, rows[:, :2].long().t().contiguous(), rows[:, 2].contiguous() if edge_weights is not None else None)

    def __call__(self, x, edge_index, edge_weight=None):
        return self.augment(Graph(x, edge_index, edge_weight))


class EdgeDropping(_EdgeDrop):
    """PyGCL's EdgeDropping(pe=p) on the device: every edge is dropped with probability p (ops.drop_edges, scheme "uniform").
    `aug(x, edge_index, edge_weight)` or `aug.augment(g)`; the edges keep their input order and their weights."""

    def __init__(self, p: float, seed: Optional[int] = None):
        super().__init__(p, 1.0, seed)


class EdgeDroppingDegree(_EdgeDrop):
    """scripts/augmentor_benchmarks.py:289-311 on the device (ops.drop_edges, scheme "degree")."""
    scheme = "degree"


class EdgeDroppingPR(_EdgeDrop):
    """scripts/augmentor_benchmarks.py:314-336 on the device (ops.drop_edges, scheme "pagerank")."""
    scheme = "pagerank"


class EdgeDroppingEVC(_EdgeDrop):
    """scripts/augmentor_benchmarks.py:339-363 on the device (ops.drop_edges, scheme "eigenvector"): the power iteration runs on the
    device instead of a round trip through networkx on the host."""
    scheme = "eigenvector"


class EdgeDroppingViews:
    """K edge-dropping views of a graph from ONE ops.drop_edges call: the centrality is found once, view k uses ps[k] and seed + k.
    `seed=None` (the default) draws a fresh seed from torch's RNG at every call, as rLapViews does; an integer seed makes every call
    return the same views; `last_seed` is the seed of the latest call.  `.augment(g)` returns the list of K graphs, `.augmentors()`
    the PyGCL-style siblings for the `(aug1, aug2)` pair of the training scripts (as rLapViews.augmentors()), `.plan(g)` one
    propagation plan over all K views for SnapshotGCNConv."""

    def __init__(self, scheme: str = "degree", ps=(0.3, 0.4), threshold: float = 0.7, seed: Optional[int] = None, aggr: str = "sink"):
        self.scheme, self.ps, self.threshold, self.seed, self.aggr = scheme, tuple(float(p) for p in ps), threshold, seed, aggr
        if len(self.ps) < 1:
            raise ValueError("ps: at least one drop parameter")
        self._pending = None
        self.last_seed = None

    def _call(self, g, **kw):
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        n = int(x.shape[0]) if x is not None else None
        self.last_seed = ops._seed_from(self.seed)
        return x, edge_weights, n, ops.drop_edges(edge_index, edge_weights, n, list(self.ps), self.scheme, self.threshold, self.last_seed, self.aggr, **kw)

    def augment(self, g):
        x, edge_weights, _, (rows, ptr) = self._call(g)
        e = ptr.tolist()
        ei = rows[:, :2].long().t().contiguous()
        return [_as_graph(x, ei[:, e[k]:e[k + 1]], rows[e[k]:e[k + 1], 2] if edge_weights is not None else None) for k in range(len(self.ps))]

    def plan(self, g, directions: str = "both", fill_value: float = 1.0):
        """One plan over all K views (layer k is view k): ops.edge_list_plan on the call's (rows, ptr), the loops covering x.shape[0]
        ids (edge_index.max() + 1 without x); weighted iff the graph has edge weights."""
        x, edge_weights, n, (rows, ptr) = self._call(g)
        if n is None:
            edge_index = g.unfold()[1] if hasattr(g, "unfold") else g[1]
            n = int(edge_index.max().item()) + 1 if edge_index.numel() else 0
        return ops.edge_list_plan(rows, ptr, n, None, edge_weights is not None, True, fill_value, True, directions)

    _key = staticmethod(rLapViews._key)
    _view = rLapViews._view

    def augmentors(self):
        return [_ViewAugmentor(self, k) for k in range(len(self.ps))]


class _NodeSample:
    """What the two node-sampling augmentors share: one ops.sample_subgraphs call, one view.  `seed=None` (the default) draws a fresh
    seed from torch's RNG at every call, as _EdgeDrop does, so the reference's `(aug1, aug2)` and two calls of one give independent
    views; an integer seed makes every call return the same view.  `last_seed` is the seed of the latest call.  num_nodes is
    edge_index.max() + 1, as PyGCL computes it: one reduction and read-back in front of the call."""
    scheme = "drop"

    def _params(self):
        raise NotImplementedError

    def augment(self, g):
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        self.last_seed = ops._seed_from(self.seed)
        rows, _ = ops.sample_subgraphs(edge_index, edge_weights, None, self.scheme, seed=self.last_seed, **self._params())
        return _as_graph(x, rows[:, :2].long().t().contiguous(), rows[:, 2].contiguous() if edge_weights is not None else None)

    def __call__(self, x, edge_index, edge_weight=None):
        return self.augment(Graph(x, edge_index, edge_weight))


class NodeDropping(_NodeSample):
    """PyGCL's NodeDropping(pn) on the device: every node is dropped with probability pn, an edge stays iff both its ends do
    (ops.sample_subgraphs, scheme "drop").  `aug(x, edge_index, edge_weight)` or `aug.augment(g)`; the edges keep their input order,
    their ids and their weights."""

    def __init__(self, pn: float, seed: Optional[int] = None):
        self.pn, self.seed, self.last_seed = pn, seed, None

    def _params(self):
        return {"p": self.pn}


class RWSampling(_NodeSample):
    """PyGCL's RWSampling(num_seeds, walk_length) on the device: the subgraph among the nodes that num_seeds uniform random walks
    of walk_length steps visit (ops.sample_subgraphs, scheme "walk")."""
    scheme = "walk"

    def __init__(self, num_seeds: int, walk_length: int = 10, seed: Optional[int] = None):
        self.num_seeds, self.walk_length, self.seed, self.last_seed = num_seeds, walk_length, seed, None

    def _params(self):
        return {"num_seeds": self.num_seeds, "walk_length": self.walk_length}


class NodeSampleViews:
    """K node-sampling views of a graph from ONE ops.sample_subgraphs call: view k uses ps_or_seeds[k] -- a drop probability for
    scheme "drop", a number of walkers for "walk" -- and seed + k.  `seed=None` (the default) draws a fresh seed from torch's RNG at
    every call, as EdgeDroppingViews does; an integer seed makes every call return the same views; `last_seed` is the seed of the
    latest call.  `.augment(g)` returns the list of K graphs, `.augmentors()` the PyGCL-style siblings for the `(aug1, aug2)` pair
    of the training scripts, `.plan(g)` one propagation plan over all K views for SnapshotGCNConv."""

    def __init__(self, scheme: str = "drop", ps_or_seeds=(0.3, 0.4), walk_length: int = 10, seed: Optional[int] = None):
        self.scheme, self.walk_length, self.seed = scheme, walk_length, seed
        self.ps = tuple(ps_or_seeds)
        if len(self.ps) < 1:
            raise ValueError("ps_or_seeds: at least one view")
        self._pending = None
        self.last_seed = None

    def _call(self, g, **kw):
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        n = int(x.shape[0]) if x is not None else None
        self.last_seed = ops._seed_from(self.seed)
        params = {"p": list(self.ps)} if self.scheme == "drop" else {"num_seeds": list(self.ps), "walk_length": self.walk_length}
        return x, edge_weights, n, ops.sample_subgraphs(edge_index, edge_weights, n, self.scheme, seed=self.last_seed, **params, **kw)

    def augment(self, g):
        x, edge_weights, _, (rows, ptr) = self._call(g)
        e = ptr.tolist()
        ei = rows[:, :2].long().t().contiguous()
        return [_as_graph(x, ei[:, e[k]:e[k + 1]], rows[e[k]:e[k + 1], 2] if edge_weights is not None else None) for k in range(len(self.ps))]

    def plan(self, g, directions: str = "both", fill_value: float = 1.0):
        """One plan over all K views (layer k is view k): ops.edge_list_plan on the call's (rows, ptr), the loops covering x.shape[0]
        ids (edge_index.max() + 1 without x); weighted iff the graph has edge weights."""
        x, edge_weights, n, (rows, ptr) = self._call(g)
        if n is None:
            edge_index = g.unfold()[1] if hasattr(g, "unfold") else g[1]
            n = int(edge_index.max().item()) + 1 if edge_index.numel() else 0
        return ops.edge_list_plan(rows, ptr, n, None, edge_weights is not None, True, fill_value, True, directions)

    _key = staticmethod(rLapViews._key)
    _view = rLapViews._view

    def augmentors(self):
        return [_ViewAugmentor(self, k) for k in range(len(self.ps))]


class EdgeAdding:
    """The EdgeAdding(pe) of the training scripts (scripts/augmentor_benchmarks.py:44-65) on the device: int(E * pe) edges with
    both ends uniform over [0, edge_index.max() - 1] -- the reference's randint has an exclusive upper end, so the last node never
    receives one -- are added, and the lot is sorted and coalesced (ops.add_edges).  `aug(x, edge_index, edge_weight)` or
    `aug.augment(g)`.  For an unweighted input the graph has no edge weights, as the reference's; for a weighted one `edge_weights`
    holds the coalesced sums, one per edge of the result (an added edge counts 1.0) -- the reference hands back the input's weight
    vector unchanged, whose length no longer matches the new edge_index.  `seed=None` (the default) draws a fresh seed from torch's
    RNG at every call, as _EdgeDrop does; an integer seed makes every call return the same view; `last_seed` is the seed of the
    latest call.  num_nodes is edge_index.max() + 1, as the reference computes it: one reduction and read-back in front of the call."""

    def __init__(self, pe: float, seed: Optional[int] = None):
        self.pe, self.seed, self.last_seed = pe, seed, None

    def augment(self, g):
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        self.last_seed = ops._seed_from(self.seed)
        rows, _ = ops.add_edges(edge_index, edge_weights, None, self.pe, self.last_seed)
        return _as_graph(x, rows[:, :2].long().t().contiguous(), rows[:, 2].contiguous() if edge_weights is not None else None)

    def __call__(self, x, edge_index, edge_weight=None):
        return self.augment(Graph(x, edge_index, edge_weight))


class EdgeAddingViews:
    """K edge-adding views of a graph from ONE ops.add_edges call: the input is sorted and coalesced once, view k adds
    int(E * pes[k]) edges and uses seed + k.  `seed=None` (the default) draws a fresh seed from torch's RNG at every call, as
    EdgeDroppingViews does; an integer seed makes every call return the same views; `last_seed` is the seed of the latest call.
    `.augment(g)` returns the list of K graphs (edge weights as EdgeAdding's), `.augmentors()` the PyGCL-style siblings for the
    `(aug1, aug2)` pair of the training scripts, `.plan(g)` one propagation plan over all K views for SnapshotGCNConv."""

    def __init__(self, pes=(0.3, 0.4), seed: Optional[int] = None):
        self.pes, self.seed = tuple(pes), seed
        if len(self.pes) < 1:
            raise ValueError("pes: at least one view")
        self._pending = None
        self.last_seed = None

    def _call(self, g, **kw):
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        n = int(x.shape[0]) if x is not None else None
        self.last_seed = ops._seed_from(self.seed)
        return x, edge_weights, n, ops.add_edges(edge_index, edge_weights, n, list(self.pes), self.last_seed, **kw)

    def augment(self, g):
        x, edge_weights, _, (rows, ptr) = self._call(g)
        e = ptr.tolist()
        ei = rows[:, :2].long().t().contiguous()
        return [_as_graph(x, ei[:, e[k]:e[k + 1]], rows[e[k]:e[k + 1], 2] if edge_weights is not None else None) for k in range(len(self.pes))]

    def plan(self, g, directions: str = "both", fill_value: float = 1.0):
        """One plan over all K views (layer k is view k): ops.edge_list_plan on the call's (rows, ptr), the loops covering x.shape[0]
        ids (edge_index.max() + 1 without x); weighted iff the graph has edge weights."""
        x, edge_weights, n, (rows, ptr) = self._call(g)
        if n is None:
            edge_index = g.unfold()[1] if hasattr(g, "unfold") else g[1]
            n = int(edge_index.max().item()) + 1 if edge_index.numel() else 0
        return ops.edge_list_plan(rows, ptr, n, None, edge_weights is not None, True, fill_value, True, directions)

    _key = staticmethod(rLapViews._key)
    _view = rLapViews._view

    def augmentors(self):
        return [_ViewAugmentor(self, k) for k in range(len(self.pes))]


def compute_ppr(edge_index: torch.Tensor, edge_weight: Optional[torch.Tensor], num_nodes: int, alpha: float = 0.2,
                eps: float = 1e-4, add_self_loop: bool = False, normalize_out: bool = True):
    """Dense personalised-PageRank diffusion, S = alpha (I - (1-alpha) D^-1/2 A D^-1/2)^-1, entries
    below `eps` dropped, then (normalize_out) the kept entries normalised symmetrically once more,
    D_S^-1/2 S D_S^-1/2 with D_S the row sums of the thresholded matrix.

    This restates PyGCL's `GCL.augmentors.functional.compute_ppr` (called by
    scripts/augmentor_benchmarks.py:152-159 with ignore_edge_attr=False, add_self_loop=False), which chains
    PyG's GDC steps: transition_matrix('sym') -> diffusion_matrix_exact('ppr') -> sparsify_dense('threshold')
    -> transition_matrix('sym').  PyGCL (pinned by the reference: requirements.txt:4, PyGCL==0.1.2) and PyG are third-party
    packages absent from this container and not installable (no network), so this row is UNPINNED: it follows the published
    semantics of those functions, not a run of them.  `normalize_out=False` gives
    the diffusion matrix before the last step.  torch ops on the input's device; meant for the sizes the
    reference uses it on (the Schur-complement subgraph)."""
    dev = edge_index.device
    w = torch.ones(edge_index.shape[1], dtype=torch.float64, device=dev) if edge_weight is None else edge_weight.to(torch.float64)
    adj = torch.zeros((num_nodes, num_nodes), dtype=torch.float64, device=dev)
    adj.index_put_((edge_index[0], edge_index[1]), w, accumulate=True)
    if add_self_loop:
        adj = adj + torch.eye(num_nodes, dtype=torch.float64, device=dev)
    deg = adj.sum(1)
    dinv = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    a_hat = dinv[:, None] * adj * dinv[None, :]
    s = alpha * torch.linalg.inv(torch.eye(num_nodes, dtype=torch.float64, device=dev) - (1 - alpha) * a_hat)
    s = torch.where(s >= eps, s, torch.zeros_like(s))
    if normalize_out:
        d2 = s.sum(1)
        d2inv = torch.where(d2 > 0, d2.pow(-0.5), torch.zeros_like(d2))
        s = d2inv[:, None] * s * d2inv[None, :]
    idx = s.nonzero(as_tuple=False).t().contiguous()
    return idx, s[idx[0], idx[1]]


def compute_markov_diffusion(edge_index: torch.Tensor, edge_weight: Optional[torch.Tensor], num_nodes: int, alpha: float = 0.2,
                             degree: int = 16, sp_eps: float = 1e-4, add_self_loop: bool = True, normalize_out: bool = False):
    """Dense Markov diffusion, M = alpha Â + (1/degree) sum_{k=0..degree} (1 - alpha)^k Â^(k+1) with Â = D^-1/2 A D^-1/2 (A + I with
    add_self_loop), entries below `sp_eps` dropped, then (normalize_out) D_M^-1/2 M D_M^-1/2 with D_M the row sums of what was kept.

    This restates PyGCL's `GCL.augmentors.functional.compute_markov_diffusion` in the published loop's order (z = Â; t = Â; `degree`
    times: t = (1 - alpha) spmm(Â, t), z += t; z /= degree; z += alpha Â; transposed -- M is symmetric -- and thresholded by
    sparsify_dense('threshold')).  PyGCL and PyG are absent from this container and not installable, so like compute_ppr this row
    is UNPINNED: it follows the published semantics as recalled, not a run of them (DESIGN.md sections 4.23 and 7).  The published
    function ends at the threshold; normalize_out=True adds compute_ppr's last step.  It is the yardstick of ops.markov_diffusion
    and the opponent of tools/markov_latency.py; torch ops on the input's device."""
    dev = edge_index.device
    w = torch.ones(edge_index.shape[1], dtype=torch.float64, device=dev) if edge_weight is None else edge_weight.to(torch.float64)
    adj = torch.zeros((num_nodes, num_nodes), dtype=torch.float64, device=dev)
    adj.index_put_((edge_index[0], edge_index[1]), w, accumulate=True)
    if add_self_loop:
        adj = adj + torch.eye(num_nodes, dtype=torch.float64, device=dev)
    deg = adj.sum(1)
    dinv = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    a_hat = dinv[:, None] * adj * dinv[None, :]
    z = a_hat.clone()
    t = a_hat.clone()
    for _ in range(int(degree)):
        t = (1.0 - alpha) * (a_hat @ t)
        z = z + t
    z = z / int(degree)
    z = z + alpha * a_hat
    z = z.t()
    z = torch.where(z >= sp_eps, z, torch.zeros_like(z))
    if normalize_out:
        d2 = z.sum(1)
        d2inv = torch.where(d2 > 0, d2.pow(-0.5), torch.zeros_like(d2))
        z = d2inv[:, None] * z * d2inv[None, :]
    idx = z.nonzero(as_tuple=False).t().contiguous()
    return idx, z[idx[0], idx[1]]


class MarkovDiffusion:
    """PyGCL's A.MarkovDiffusion (restated, unpinned as compute_markov_diffusion is) on the device: ops.markov_diffusion of the
    graph's edge list, cached after the first call when `use_cache` as PyGCL's is (the graph-level scripts pass use_cache=False and
    diffuse every batch).  `node_ptr` -- node_ptr_of(batch) for a collated batch -- diffuses every graph of the batch on its own in
    the one call.  num_nodes is x.shape[0] when x is given, else edge_index.max() + 1."""

    def __init__(self, alpha: float = 0.05, order: int = 16, sp_eps: float = 1e-4, use_cache: bool = True, add_self_loop: bool = True):
        self.alpha, self.order, self.sp_eps = alpha, order, sp_eps
        self.use_cache, self.add_self_loop = use_cache, add_self_loop
        self._cache = None

    def augment(self, g, node_ptr=None):
        if self._cache is not None and self.use_cache:
            return self._cache
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        if x is not None:
            n = int(x.shape[0])
        elif node_ptr is not None:
            n = int(torch.as_tensor(node_ptr)[-1])
        else:
            n = int(edge_index.max().item()) + 1 if edge_index.numel() else 0
        ei, w = ops.markov_diffusion(edge_index, edge_weights, n, node_ptr=node_ptr, alpha=self.alpha, order=self.order,
                                     eps=self.sp_eps, add_self_loop=self.add_self_loop)
        res = _as_graph(x, ei, w)
        self._cache = res
        return res

    def __call__(self, x, edge_index, edge_weight=None, node_ptr=None):
        return self.augment(Graph(x, edge_index, edge_weight), node_ptr=node_ptr)


class rLapPPRDiffusion:
    """scripts/augmentor_benchmarks.py:99-171: Schur complement (weights kept) -> induced subgraph on
    the surviving nodes, relabelled -> PPR diffusion -> original ids; result cached for
    `refresh_cache_freq` calls like the reference."""

    def __init__(self, frac, o_v="random", o_n="asc", alpha=0.2, eps=1e-4, use_cache=True, refresh_cache_freq=50, seed=None,
                 num_nodes_from_x=False, normalize_out=True, weights_dtype=torch.float64):
        self.frac, self.o_v, self.o_n, self.alpha, self.eps = frac, o_v, o_n, alpha, eps
        self.use_cache, self.refresh_cache_freq = use_cache, refresh_cache_freq
        self._cache, self.refresh_cache_counter, self.seed = None, 0, seed
        self.num_nodes_from_x, self.normalize_out = num_nodes_from_x, normalize_out
        # The reference hands compute_ppr `torch.Tensor(sparse_edge_info[:, -1])` (augmentor_benchmarks.py:144-146).  On the torch of
        # this image (2.10) that expression keeps float64 (checked: torch.Tensor(f64 tensor).dtype is float64); on the legacy
        # constructor of older torch builds it is the default tensor type, float32.  float64 is the default here;
        # weights_dtype=torch.float32 rounds the Schur-complement weights once before the diffusion, as such a build would.
        self.weights_dtype = weights_dtype

    def augment(self, g):
        if self._cache is not None and self.use_cache and self.refresh_cache_counter < self.refresh_cache_freq:
            self.refresh_cache_counter += 1
            return self._cache
        x, edge_index, edge_weights = g.unfold() if hasattr(g, "unfold") else g
        sc, num_nodes = _schur(edge_index, edge_weights, x, self.frac, self.o_v, self.o_n, self.seed, self.num_nodes_from_x, False)
        self.num_remove = int(self.frac * num_nodes)
        ei = sc[:, :2].long().t()
        nodes = torch.unique(ei, sorted=True)                       # surviving nodes that still have edges
        relabel = torch.full((num_nodes,), -1, dtype=torch.int64, device=ei.device)
        relabel[nodes] = torch.arange(nodes.numel(), device=ei.device)
        sub_ei = relabel[ei]
        d_ei, d_w = compute_ppr(sub_ei, sc[:, 2].to(self.weights_dtype), nodes.numel(), alpha=self.alpha, eps=self.eps, normalize_out=self.normalize_out)
        res = Graph(x, nodes[d_ei], d_w)
        self._cache, self.refresh_cache_counter = res, 0
        return res

    def __call__(self, x, edge_index, edge_weight=None):
        return self.augment(Graph(x, edge_index, edge_weight))


class rLapDGL:
    """DGL-style augmentor (CCA-SSG/aug.py:33-63): edges -> (2,E) -> op (edge_weights=None) -> new graph."""

    def __init__(self, frac: float, o_v: str = "random", o_n: str = "asc", seed: Optional[int] = None):
        self.frac = frac
        self.o_v = o_v
        self.o_n = o_n
        self.seed = seed

    def augment(self, graph):
        try:
            import dgl  # type: ignore
        except ImportError:
            dgl = None
        if dgl is not None and hasattr(graph, "edges"):
            src, dst = graph.edges()
            num_nodes = graph.num_nodes()
        else:  # (edge_index, num_nodes) stand-in
            edge_index, num_nodes = graph
            src, dst = edge_index[0], edge_index[1]
        edge_index = torch.stack([src, dst])
        sc = ops.approximate_cholesky(edge_index, None, num_nodes, int(self.frac * num_nodes), self.o_v, self.o_n,
                                      seed=self.seed, return_device="same")
        ei = sc[:, :2].long().t()
        if dgl is not None and hasattr(graph, "edges"):
            return dgl.graph((ei[0], ei[1]), num_nodes=num_nodes)
        return ei, num_nodes


def get_split(num_samples: int, train_ratio: float = 0.1, test_ratio: float = 0.8, runs: Optional[int] = None, generator=None):
    """PyGCL's get_split (GCL/eval/eval.py), restated from the published text -- PyGCL is not a dependency, as SnapshotGCNConv
    restates PyG's layer: a randperm of the rows is cut at int(n * train_ratio) and int(n * test_ratio); 'train' is the first
    train_size rows, 'valid' the NEXT test_size rows and 'test' the rest, exactly as published (so with the defaults 'valid' holds
    80 % of the rows and 'test' 10 %).  runs=R returns a list of R splits drawn one after the other from `generator`."""
    assert train_ratio + test_ratio < 1
    train_size = int(num_samples * train_ratio)
    test_size = int(num_samples * test_ratio)

    def one():
        indices = torch.randperm(num_samples, generator=generator)
        return {"train": indices[:train_size], "valid": indices[train_size: test_size + train_size], "test": indices[test_size + train_size:]}

    return one() if runs is None else [one() for _ in range(int(runs))]


class LREvaluator:
    """The reference's LREvaluator (scripts/node_shared.py:163-230) on ops.linear_probe: evaluate(x, y, split) returns its dict of
    Python floats {"micro_f1", "macro_f1", "accuracy"}; reading them is the one host synchronisation.  evaluate_runs(x, y, splits)
    takes a list of splits -- the ten of a test() loop, say --, makes ONE call and returns the list of dicts.  select="cca" applies
    CCA-SSG/main.py:172-186's rule instead.  The initial parameters are drawn as the reference draws them, from `generator`."""

    def __init__(self, num_epochs: int = 2000, learning_rate: float = 0.01, weight_decay: float = 0.0, test_interval: int = 20,
                 select: str = "scripts", generator=None):
        self.num_epochs = num_epochs
        self.learning_rate = learning_rate
        self.weight_decay = weight_decay
        self.test_interval = test_interval
        self.select = select
        self.generator = generator
        self.last = None   # the device result of the last call

    def evaluate_runs(self, x: torch.Tensor, y: torch.Tensor, splits) -> list:
        splits = list(splits)
        res = ops.linear_probe(x, y, [s["train"] for s in splits], [s["valid"] for s in splits], [s["test"] for s in splits],
                               epochs=self.num_epochs, lr=self.learning_rate, weight_decay=self.weight_decay,
                               test_interval=self.test_interval, select=self.select, generator=self.generator)
        self.last = res
        status = int(res["status"])   # (the synchronisation)
        if status != 0:
            raise ValueError("LREvaluator: " + ("an index outside [0, N)" if status == 2 else "a label outside [0, num_classes)"))
        micro, macro, acc = res["micro_f1"].tolist(), res["macro_f1"].tolist(), res["accuracy"].tolist()
        return [{"micro_f1": micro[r], "macro_f1": macro[r], "accuracy": acc[r]} for r in range(len(splits))]

    def evaluate(self, x: torch.Tensor, y: torch.Tensor, split: dict) -> dict:
        return self.evaluate_runs(x, y, [split])[0]

    def __call__(self, x: torch.Tensor, y: torch.Tensor, split: dict) -> dict:
        return self.evaluate(x, y, split)
