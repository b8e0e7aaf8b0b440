"""ctypes loader for librlap_hip.so (the C ABI in include/rlap_hip.h).

The product path has no CPU fallback: if the HIP library is missing, or no GPU is
visible, calls raise instead of silently computing somewhere else.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RLAP_AMD_LIB") or os.path.join(_HERE, "librlap_hip.so")   # (override: kernel-variant experiments)

_lib = None

# every symbol include/rlap_hip.h declares
EXPORTS = [
    "rlap_create", "rlap_destroy", "rlap_set_stream", "rlap_set_timing", "rlap_status_string",
    "rlap_identity", "rlap_unpack_edge_info", "rlap_approx_chol", "rlap_approx_chol_batched",
    "rlap_rng_uniforms", "rlap_util_ba_graph", "rlap_debug_wave_sort",
    "rlap_approx_chol_from_edges", "rlap_debug_set_limits", "rlap_pack_rows", "rlap_unpack_rows",
    "rlap_workspace_bytes", "rlap_workspace_query", "rlap_set_workspace", "rlap_workspace_needed", "rlap_debug_set_poison", "rlap_debug_set_jitter",
    "rlap_set_rng_mode", "rlap_approx_chol_views", "rlap_approx_chol_depths", "rlap_debug_set_flow_limits",
    "rlap_approx_chol_views_depths", "rlap_snapshot_stats", "rlap_snapshot_ppr", "rlap_snapshot_subgraph",
    "rlap_snapshot_gcn_norm", "rlap_snapshot_propagate",
    "rlap_snapshot_plan_bytes", "rlap_snapshot_plan_build", "rlap_snapshot_plan_propagate", "rlap_edge_plan_build",
    "rlap_graph_readout", "rlap_graph_readout_backward", "rlap_infonce", "rlap_infonce_backward",
    "rlap_infonce_pair", "rlap_infonce_pair_backward",
    "rlap_infonce_intra", "rlap_infonce_intra_backward", "rlap_infonce_pair_intra", "rlap_infonce_pair_intra_backward",
    "rlap_cca_loss", "rlap_cca_loss_backward", "rlap_bt_loss", "rlap_bt_loss_backward", "rlap_batch_norm", "rlap_batch_norm_backward",
    "rlap_g2l_jsd", "rlap_g2l_jsd_backward", "rlap_g2l_bootstrap", "rlap_g2l_bootstrap_backward",
    "rlap_linear_probe", "rlap_probe_scores", "rlap_edge_drop", "rlap_node_sample", "rlap_edge_add", "rlap_snapshot_markov",
    "rlap_feature_count", "rlap_feature_plan_bytes", "rlap_feature_plan_build", "rlap_feature_plan_apply",
    "rlap_bias_act_dropout", "rlap_bias_act_dropout_backward", "rlap_layer_norm", "rlap_layer_norm_backward",
    "rlap_linear_act", "rlap_linear_act_backward",
]

E_INDEX_RANGE = 2   # RLAP_E_INDEX_RANGE
E_WORKSPACE = 11   # RLAP_E_WORKSPACE
E_NOT_GROUPED = 12   # RLAP_E_NOT_GROUPED
E_OUT_CAPACITY = 13   # RLAP_E_OUT_CAPACITY
# rlap_snapshot_ppr flags
PPR_WEIGHTED, PPR_SELF_LOOP, PPR_NORMALIZE, PPR_ZERO_ROWS = 1, 2, 4, 8
# rlap_snapshot_markov flags and limits (rlap_amd/csrc/rlap_markov.h)
MARKOV_WEIGHTED, MARKOV_SELF_LOOP, MARKOV_NORMALIZE, MARKOV_ZERO_ROWS = 1, 2, 4, 8
MARKOV_MAX_ORDER = 1024
# rlap_snapshot_subgraph flags
SUB_RELABEL, SUB_NO_SELF_LOOPS = 1, 2
# rlap_snapshot_gcn_norm flags
GCN_WEIGHTED, GCN_SELF_LOOPS, GCN_NORMALIZE, GCN_F32 = 1, 2, 4, 8
# rlap_snapshot_propagate flags (beside the first three above)
SPMM_TRANSPOSE, SPMM_X_F32, SPMM_X_PER_LAYER = 16, 32, 64
# rlap_snapshot_plan_build flags (beside the first three of rlap_snapshot_gcn_norm): the directions to build
PLAN_FORWARD, PLAN_TRANSPOSED = 256, 512
PLAN_MAGIC = 0x504C414E   # rlap_plan_desc.magic of a successful build
# rlap_feature_plan_build flags (beside the two directions above) and limits (rlap_amd/csrc/rlap_featlin.h)
FEAT_X_F32 = 1
FEAT_MAGIC = 0x46454154   # rlap_feature_desc.magic of a successful build
FEAT_MAX_VIEWS = 32
# rlap_edge_drop schemes and flags
DROP_SCHEMES = {"uniform": 0, "degree": 1, "pagerank": 2, "eigenvector": 3}
DROP_SOURCE = 1
DROP_MAX_VIEWS = 32
# rlap_node_sample schemes and limits
SAMPLE_SCHEMES = {"drop": 0, "walk": 1}
SAMPLE_MAX_WALK_LENGTH = 1024
SAMPLE_MAX_SEEDS = 2**31 - 1
# rlap_edge_add flags and limits
ADD_COALESCE = 1
ADD_MAX_ROWS = 2**31 - 2   # E + the largest num_add
# rlap_graph_readout flags
READOUT_MEAN, READOUT_X_F32 = 1, 32
# rlap_infonce flags
INFONCE_POSITIVE_RAW = 1
# the intraview argument of rlap_infonce_intra and its kin
INFONCE_INTRA_MASKED, INFONCE_INTRA_ALL = 1, 2
# rlap_batch_norm flags and limits (rlap_amd/csrc/rlap_norm.h)
NORM_PRE_RELU, NORM_POST_RELU, NORM_POST_PRELU, NORM_SLOPE_PER_CHANNEL, NORM_EVAL = 1, 2, 4, 8, 16
NORM_MAX_F = 4096
# rlap_bias_act_dropout flags and limits (rlap_amd/csrc/rlap_rowops.h)
ROW_ACT_RELU, ROW_ACT_PRELU, ROW_SLOPE_PER_CHANNEL, ROW_TRAINING = 1, 2, 4, 8
ROW_MAX_F = 4096
# rlap_linear_act flags, activations and limits (rlap_amd/csrc/rlap_linear.h)
LINEAR_WEIGHT_OUT_IN = 1
LINEAR_ACT_NONE, LINEAR_ACT_RELU, LINEAR_ACT_ELU = 0, 1, 2
LINEAR_MAX_F = 512
# rlap_linear_probe select
PROBE_SELECT_SCRIPTS, PROBE_SELECT_CCA = 0, 1

# rlap_stats.elim_kernel
KERNEL_NONE, KERNEL_ROUND, KERNEL_FLOW = 0, 1, 2
# rlap_stats.retry_causes: bit k = retry kind k (include/rlap_hip.h)
RETRY_POOL, RETRY_LOG, RETRY_RNG, RETRY_SCRATCH, RETRY_SORT, RETRY_FLOW_SCRATCH, RETRY_FLOW_REORDER, RETRY_FLOW_GAVE_UP = (1 << k for k in range(1, 9))
# rlap_stats.flow_abort
FLOW_ABORT_REASONS = {0: "none", 1: "stall watchdog", 2: "sorted-index check", 3: "appended count over 2^22", 4: "column longer than its buffer"}


class _Report(ctypes.Structure):
    """What a call writes for its caller: rlap_stats and the info structures of the snapshot calls (include/rlap_hip.h)."""

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "pad"}


class Stats(_Report):
    _fields_ = [
        ("nnz", ctypes.c_int64), ("n_eliminated", ctypes.c_int64), ("n_draws", ctypes.c_int64),
        ("out_rows", ctypes.c_int64), ("live_entries", ctypes.c_int64),
        ("ms_setup", ctypes.c_float), ("ms_elim", ctypes.c_float), ("ms_output", ctypes.c_float),
        ("ms_sc_merge", ctypes.c_float), ("ms_sc_compact", ctypes.c_float), ("ms_total", ctypes.c_float),
        ("n_retries", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("n_rounds", ctypes.c_int64), ("n_singles", ctypes.c_int64),
        ("elim_kernel", ctypes.c_int32), ("retry_causes", ctypes.c_int32), ("flow_abort", ctypes.c_int32), ("n_rounds_narrow", ctypes.c_int32),
        ("n_squeezes", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class SnapshotInfo(_Report):
    """rlap_snapshot_info (include/rlap_hip.h)."""
    _fields_ = [
        ("small_segments", ctypes.c_int64), ("large_segments", ctypes.c_int64), ("lanczos_steps", ctypes.c_int64),
        ("large_steps", ctypes.c_int64), ("large_launches", ctypes.c_int64), ("host_syncs", ctypes.c_int32),
        ("not_converged", ctypes.c_int32),
    ]


class PprInfo(_Report):
    """rlap_ppr_info (include/rlap_hip.h)."""
    _fields_ = [
        ("steps", ctypes.c_int64), ("small_tiles", ctypes.c_int64), ("large_tiles", ctypes.c_int64), ("groups", ctypes.c_int64),
        ("launches", ctypes.c_int64), ("rows_needed", ctypes.c_int64), ("arena_bytes", ctypes.c_int64), ("host_syncs", ctypes.c_int32),
        ("pad", ctypes.c_int32),
    ]


class MarkovInfo(_Report):
    """rlap_markov_info (include/rlap_hip.h)."""
    _fields_ = [
        ("order", ctypes.c_int64), ("small_tiles", ctypes.c_int64), ("large_tiles", ctypes.c_int64),
        ("groups", ctypes.c_int64), ("launches", ctypes.c_int64), ("rows_needed", ctypes.c_int64), ("arena_bytes", ctypes.c_int64),
        ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class SubgraphInfo(_Report):
    """rlap_subgraph_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows_kept", ctypes.c_int64), ("ids_written", ctypes.c_int64), ("arena_bytes", ctypes.c_int64), ("host_syncs", ctypes.c_int32),
        ("pad", ctypes.c_int32),
    ]


class GcnInfo(_Report):
    """rlap_gcn_info (include/rlap_hip.h)."""
    _fields_ = [
        ("entries", ctypes.c_int64), ("loops_removed", ctypes.c_int64), ("arena_bytes", ctypes.c_int64), ("host_syncs", ctypes.c_int32),
        ("pad", ctypes.c_int32),
    ]


class SpmmInfo(_Report):
    """rlap_spmm_info (include/rlap_hip.h)."""
    _fields_ = [
        ("entries", ctypes.c_int64), ("blocks", ctypes.c_int64), ("chunked_lists", ctypes.c_int64), ("arena_bytes", ctypes.c_int64),
        ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class PlanDesc(_Report):
    """rlap_plan_desc (include/rlap_hip.h)."""
    _fields_ = [
        ("m", ctypes.c_int64), ("segments", ctypes.c_int64), ("graphs", ctypes.c_int64), ("num_nodes", ctypes.c_int64),
        ("fill_value", ctypes.c_double),
        ("entries_forward", ctypes.c_int64), ("entries_transposed", ctypes.c_int64),
        ("chunks_forward", ctypes.c_int64), ("chunks_transposed", ctypes.c_int64),
        ("loop_offset", ctypes.c_int64),
        ("off_forward", ctypes.c_int64), ("dir_forward", ctypes.c_int64), ("rec_forward", ctypes.c_int64),
        ("off_transposed", ctypes.c_int64), ("dir_transposed", ctypes.c_int64), ("rec_transposed", ctypes.c_int64),
        ("plan_bytes", ctypes.c_int64), ("flags", ctypes.c_int32), ("magic", ctypes.c_int32),
    ]


class PlanInfo(_Report):
    """rlap_plan_info (include/rlap_hip.h)."""
    _fields_ = [
        ("entries", ctypes.c_int64), ("blocks", ctypes.c_int64), ("chunked_lists_forward", ctypes.c_int64),
        ("chunked_lists_transposed", ctypes.c_int64), ("loops_removed", ctypes.c_int64), ("arena_bytes", ctypes.c_int64),
        ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class FeatureDesc(_Report):
    """rlap_feature_desc (include/rlap_hip.h)."""
    _fields_ = [
        ("num_nodes", ctypes.c_int64), ("in_features", ctypes.c_int64), ("nnz", ctypes.c_int64),
        ("chunks_forward", ctypes.c_int64), ("chunks_transposed", ctypes.c_int64),
        ("off_forward", ctypes.c_int64), ("dir_forward", ctypes.c_int64), ("rec_forward", ctypes.c_int64),
        ("off_transposed", ctypes.c_int64), ("dir_transposed", ctypes.c_int64), ("rec_transposed", ctypes.c_int64),
        ("plan_bytes", ctypes.c_int64), ("flags", ctypes.c_int32), ("magic", ctypes.c_int32),
    ]


class FeatureInfo(_Report):
    """rlap_feature_info (include/rlap_hip.h)."""
    _fields_ = [
        ("nnz", ctypes.c_int64), ("longest_forward", ctypes.c_int64), ("longest_transposed", ctypes.c_int64),
        ("long_lists_forward", ctypes.c_int64), ("long_lists_transposed", ctypes.c_int64),
        ("chunks_forward", ctypes.c_int64), ("chunks_transposed", ctypes.c_int64), ("arena_bytes", ctypes.c_int64),
        ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class ReadoutInfo(_Report):
    """rlap_readout_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows", ctypes.c_int64), ("graphs", ctypes.c_int64), ("chunks", ctypes.c_int64), ("chunked_graphs", ctypes.c_int64),
        ("arena_bytes", ctypes.c_int64), ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class InfonceInfo(_Report):
    """rlap_infonce_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows", ctypes.c_int64), ("features", ctypes.c_int64), ("parts", ctypes.c_int64), ("arena_bytes", ctypes.c_int64),
        ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class InfoncePairInfo(_Report):
    """rlap_infonce_pair_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows", ctypes.c_int64), ("features", ctypes.c_int64), ("arena_bytes", ctypes.c_int64), ("parts", ctypes.c_int64),
        ("groups", ctypes.c_int64), ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class CcaInfo(_Report):
    """rlap_cca_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows", ctypes.c_int64), ("features", ctypes.c_int64), ("parts", ctypes.c_int64), ("arena_bytes", ctypes.c_int64),
        ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class BtInfo(_Report):
    """rlap_bt_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows", ctypes.c_int64), ("features", ctypes.c_int64), ("parts", ctypes.c_int64), ("arena_bytes", ctypes.c_int64),
        ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class LinearInfo(_Report):
    """rlap_linear_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows", ctypes.c_int64), ("fin", ctypes.c_int64), ("fout", ctypes.c_int64), ("parts", ctypes.c_int64),
        ("arena_bytes", ctypes.c_int64), ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class NormInfo(_Report):
    """rlap_norm_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows", ctypes.c_int64), ("features", ctypes.c_int64), ("layers", ctypes.c_int64), ("chunks", ctypes.c_int64),
        ("arena_bytes", ctypes.c_int64), ("vec", ctypes.c_int32), ("launches", ctypes.c_int32), ("host_syncs", ctypes.c_int32),
        ("pad", ctypes.c_int32),
    ]


class RowopsInfo(_Report):
    """rlap_rowops_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows", ctypes.c_int64), ("features", ctypes.c_int64), ("layers", ctypes.c_int64), ("chunks", ctypes.c_int64),
        ("arena_bytes", ctypes.c_int64), ("vec", ctypes.c_int32), ("launches", ctypes.c_int32), ("instance", ctypes.c_int32),
        ("host_syncs", ctypes.c_int32),
    ]


class G2lInfo(_Report):
    """rlap_g2l_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows", ctypes.c_int64), ("graphs", ctypes.c_int64), ("features", ctypes.c_int64), ("parts", ctypes.c_int64),
        ("arena_bytes", ctypes.c_int64), ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class ProbeInfo(_Report):
    """rlap_probe_info (include/rlap_hip.h)."""
    _fields_ = [
        ("runs", ctypes.c_int64), ("parts", ctypes.c_int64), ("launches", ctypes.c_int64), ("arena_bytes", ctypes.c_int64),
        ("host_syncs", ctypes.c_int32), ("detail", ctypes.c_int32),
    ]


class EdgeDropInfo(_Report):
    """rlap_edge_drop_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows_needed", ctypes.c_int64), ("launches", ctypes.c_int64), ("arena_bytes", ctypes.c_int64), ("iters", ctypes.c_int32),
        ("converged", ctypes.c_int32), ("host_syncs", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class NodeSampleInfo(_Report):
    """rlap_node_sample_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows_needed", ctypes.c_int64), ("launches", ctypes.c_int64), ("arena_bytes", ctypes.c_int64), ("host_syncs", ctypes.c_int32),
        ("pad", ctypes.c_int32),
    ]


class EdgeAddInfo(_Report):
    """rlap_edge_add_info (include/rlap_hip.h)."""
    _fields_ = [
        ("rows_needed", ctypes.c_int64), ("added", ctypes.c_int64), ("input_distinct", ctypes.c_int64), ("launches", ctypes.c_int64),
        ("arena_bytes", ctypes.c_int64), ("input_sorted", ctypes.c_int32), ("sorts", ctypes.c_int32), ("host_syncs", ctypes.c_int32),
        ("pad", ctypes.c_int32),
    ]


def load():
    """dlopen the library and declare prototypes. Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"rlap_amd: {LIB_PATH} is missing. Build it with `make -C rlap_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    vp, i64, u64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int
    lib.rlap_create.restype = ci
    lib.rlap_create.argtypes = [ctypes.POINTER(vp)]
    lib.rlap_destroy.restype = ci
    lib.rlap_destroy.argtypes = [vp]
    lib.rlap_set_stream.restype = ci
    lib.rlap_set_stream.argtypes = [vp, vp]
    lib.rlap_set_timing.restype = ci
    lib.rlap_set_timing.argtypes = [vp, ci]
    lib.rlap_status_string.restype = ctypes.c_char_p
    lib.rlap_status_string.argtypes = [ci]
    lib.rlap_identity.restype = ci
    lib.rlap_identity.argtypes = [vp, vp, vp, vp, i64, i64]
    lib.rlap_unpack_edge_info.restype = ci
    lib.rlap_unpack_edge_info.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.rlap_approx_chol.restype = ci
    lib.rlap_approx_chol.argtypes = [vp, vp, vp, vp, i64, i64, i64, ci, ci, vp, u64, vp, i64,
                                     ctypes.POINTER(i64), ctypes.POINTER(Stats)]
    lib.rlap_approx_chol_batched.restype = ci
    lib.rlap_approx_chol_batched.argtypes = [vp, vp, vp, vp, i64, i64, vp, vp, ci, ci, vp, u64, vp, i64, vp,
                                             ctypes.POINTER(Stats)]
    lib.rlap_approx_chol_depths.restype = ci
    lib.rlap_approx_chol_depths.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, ci, ci, vp, u64, vp, i64, vp, ctypes.POINTER(Stats)]
    lib.rlap_approx_chol_views_depths.restype = ci
    lib.rlap_approx_chol_views_depths.argtypes = [vp, vp, vp, vp, i64, i64, vp, i64, i64, vp, ci, ci, vp, u64, vp, i64, vp,
                                                  ctypes.POINTER(Stats)]
    lib.rlap_snapshot_stats.restype = ci
    lib.rlap_snapshot_stats.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, ci, ctypes.c_double, ctypes.c_int32, vp, vp, vp, vp,
                                        ctypes.POINTER(SnapshotInfo)]
    lib.rlap_snapshot_ppr.restype = ci
    lib.rlap_snapshot_ppr.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, ci, vp, i64,
                                      vp, ctypes.POINTER(PprInfo)]
    lib.rlap_snapshot_markov.restype = ci
    lib.rlap_snapshot_markov.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, ctypes.c_double, ctypes.c_int32, ctypes.c_double, ci, vp, i64,
                                         vp, ctypes.POINTER(MarkovInfo)]
    lib.rlap_snapshot_subgraph.restype = ci
    lib.rlap_snapshot_subgraph.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, vp, vp, i64, ci, vp, vp, vp, i64, vp,
                                           ctypes.POINTER(SubgraphInfo)]
    lib.rlap_snapshot_gcn_norm.restype = ci
    lib.rlap_snapshot_gcn_norm.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, ci, ctypes.c_double, vp, vp, vp, i64, vp,
                                           ctypes.POINTER(GcnInfo)]
    lib.rlap_snapshot_propagate.restype = ci
    lib.rlap_snapshot_propagate.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, ci, ctypes.c_double, vp, i64, vp,
                                            ctypes.POINTER(SpmmInfo)]
    lib.rlap_snapshot_plan_bytes.restype = ci
    lib.rlap_snapshot_plan_bytes.argtypes = [i64, i64, i64, i64, ci, ctypes.POINTER(ctypes.c_size_t)]
    lib.rlap_snapshot_plan_build.restype = ci
    lib.rlap_snapshot_plan_build.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, ci, ctypes.c_double, vp, ctypes.c_size_t,
                                             ctypes.POINTER(PlanDesc), ctypes.POINTER(PlanInfo)]
    lib.rlap_edge_plan_build.restype = ci
    lib.rlap_edge_plan_build.argtypes = lib.rlap_snapshot_plan_build.argtypes
    lib.rlap_snapshot_plan_propagate.restype = ci
    lib.rlap_snapshot_plan_propagate.argtypes = [vp, vp, ctypes.POINTER(PlanDesc), ci, vp, i64, vp, ctypes.POINTER(SpmmInfo)]
    lib.rlap_feature_count.restype = ci
    lib.rlap_feature_count.argtypes = [vp, vp, i64, i64, ci, ctypes.POINTER(i64)]
    lib.rlap_feature_plan_bytes.restype = ci
    lib.rlap_feature_plan_bytes.argtypes = [i64, i64, i64, ci, ctypes.POINTER(ctypes.c_size_t)]
    lib.rlap_feature_plan_build.restype = ci
    lib.rlap_feature_plan_build.argtypes = [vp, vp, i64, i64, i64, ci, vp, ctypes.c_size_t, ctypes.POINTER(FeatureDesc),
                                            ctypes.POINTER(FeatureInfo)]
    lib.rlap_feature_plan_apply.restype = ci
    lib.rlap_feature_plan_apply.argtypes = [vp, vp, ctypes.POINTER(FeatureDesc), ci, vp, vp, i64, i64, vp, ctypes.POINTER(FeatureInfo)]
    lib.rlap_graph_readout.restype = ci
    lib.rlap_graph_readout.argtypes = [vp, vp, i64, i64, i64, vp, i64, ci, vp, ctypes.POINTER(ReadoutInfo)]
    lib.rlap_graph_readout_backward.restype = ci
    lib.rlap_graph_readout_backward.argtypes = lib.rlap_graph_readout.argtypes
    lib.rlap_infonce.restype = ci
    lib.rlap_infonce.argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ci, vp, vp, vp, ctypes.POINTER(InfonceInfo)]
    lib.rlap_infonce_backward.restype = ci
    lib.rlap_infonce_backward.argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ci, vp, vp, vp, vp, ctypes.POINTER(InfonceInfo)]
    lib.rlap_infonce_pair.restype = ci
    lib.rlap_infonce_pair.argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ci, vp, vp, vp, ctypes.POINTER(InfoncePairInfo)]
    lib.rlap_infonce_pair_backward.restype = ci
    lib.rlap_infonce_pair_backward.argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ci, vp, vp, vp, vp, ctypes.POINTER(InfoncePairInfo)]
    for name, info in (("rlap_infonce_intra", InfonceInfo), ("rlap_infonce_pair_intra", InfoncePairInfo)):   # `intraview` behind `flags`
        getattr(lib, name).restype = ci
        getattr(lib, name).argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ci, ci, vp, vp, vp, ctypes.POINTER(info)]
        getattr(lib, name + "_backward").restype = ci
        getattr(lib, name + "_backward").argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ci, ci, vp, vp, vp, vp, ctypes.POINTER(info)]
    lib.rlap_cca_loss.restype = ci
    lib.rlap_cca_loss.argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ci, vp, vp, vp, ctypes.POINTER(CcaInfo)]
    lib.rlap_cca_loss_backward.restype = ci
    lib.rlap_cca_loss_backward.argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ci, vp, vp, vp, vp, vp, ctypes.POINTER(CcaInfo)]
    lib.rlap_bt_loss.restype = ci
    lib.rlap_bt_loss.argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ctypes.c_double, ci, vp, vp, vp, ctypes.POINTER(BtInfo)]
    lib.rlap_bt_loss_backward.restype = ci
    lib.rlap_bt_loss_backward.argtypes = [vp, vp, vp, i64, i64, ctypes.c_double, ctypes.c_double, ci, vp, vp, vp, vp, vp, ctypes.POINTER(BtInfo)]
    lib.rlap_linear_act.restype = ci
    lib.rlap_linear_act.argtypes = [vp, vp, i64, i64, i64, vp, vp, ci, ctypes.c_double, ci, vp, ctypes.POINTER(LinearInfo)]
    lib.rlap_linear_act_backward.restype = ci
    lib.rlap_linear_act_backward.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, ci, ctypes.c_double, ci, vp, vp, vp, ctypes.POINTER(LinearInfo)]
    lib.rlap_batch_norm.restype = ci
    lib.rlap_batch_norm.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, ctypes.c_double, ctypes.c_double, ci, vp, vp,
                                    ctypes.POINTER(NormInfo)]
    lib.rlap_batch_norm_backward.restype = ci
    lib.rlap_batch_norm_backward.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, ctypes.c_double, ci, vp, vp, vp, vp, vp,
                                             ctypes.POINTER(NormInfo)]
    lib.rlap_bias_act_dropout.restype = ci
    lib.rlap_bias_act_dropout.argtypes = [vp, vp, i64, i64, i64, vp, vp, ctypes.c_double, u64, ci, vp, ctypes.POINTER(RowopsInfo)]
    lib.rlap_bias_act_dropout_backward.restype = ci
    lib.rlap_bias_act_dropout_backward.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, ctypes.c_double, u64, ci, vp, vp, vp,
                                                   ctypes.POINTER(RowopsInfo)]
    lib.rlap_layer_norm.restype = ci
    lib.rlap_layer_norm.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, ctypes.c_double, ctypes.c_double, u64, ci, vp, ctypes.POINTER(RowopsInfo)]
    lib.rlap_layer_norm_backward.restype = ci
    lib.rlap_layer_norm_backward.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, vp, ctypes.c_double, ctypes.c_double, u64, ci, vp, vp, vp, vp,
                                             ctypes.POINTER(RowopsInfo)]
    lib.rlap_g2l_jsd.restype = ci
    lib.rlap_g2l_jsd.argtypes = [vp, vp, vp, vp, i64, i64, vp, i64, ci, vp, vp, ctypes.POINTER(G2lInfo)]
    lib.rlap_g2l_jsd_backward.restype = ci
    lib.rlap_g2l_jsd_backward.argtypes = [vp, vp, vp, vp, i64, i64, vp, i64, ci, vp, vp, vp, vp, ctypes.POINTER(G2lInfo)]
    lib.rlap_g2l_bootstrap.restype = ci
    lib.rlap_g2l_bootstrap.argtypes = [vp, vp, vp, i64, i64, vp, i64, ci, vp, vp, ctypes.POINTER(G2lInfo)]
    lib.rlap_g2l_bootstrap_backward.restype = ci
    lib.rlap_g2l_bootstrap_backward.argtypes = [vp, vp, vp, i64, i64, vp, i64, ci, vp, vp, ctypes.POINTER(G2lInfo)]
    dbl = ctypes.c_double
    lib.rlap_linear_probe.restype = ci
    lib.rlap_linear_probe.argtypes = [vp, vp, i64, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, dbl, dbl, i64, ci, dbl, dbl, dbl,
                                      vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(ProbeInfo)]
    lib.rlap_probe_scores.restype = ci
    lib.rlap_probe_scores.argtypes = [vp, vp, i64, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(ProbeInfo)]
    lib.rlap_edge_drop.restype = ci
    lib.rlap_edge_drop.argtypes = [vp, vp, vp, vp, i64, i64, ci, ci, ctypes.POINTER(dbl), i64, dbl, u64, dbl, i64, dbl, i64, vp, i64, vp, vp, vp, vp,
                                   ctypes.POINTER(EdgeDropInfo)]
    lib.rlap_node_sample.restype = ci
    lib.rlap_node_sample.argtypes = [vp, vp, vp, vp, i64, i64, ci, ctypes.POINTER(dbl), ctypes.POINTER(i64), i64, i64, u64, vp, i64, vp, vp, vp,
                                     ctypes.POINTER(NodeSampleInfo)]
    lib.rlap_edge_add.restype = ci
    lib.rlap_edge_add.argtypes = [vp, vp, vp, vp, i64, i64, ctypes.POINTER(i64), i64, u64, ci, vp, i64, vp, vp, vp, ctypes.POINTER(EdgeAddInfo)]
    lib.rlap_approx_chol_views.restype = ci
    lib.rlap_approx_chol_views.argtypes = [vp, vp, vp, vp, i64, i64, vp, i64, vp, ci, ci, vp, u64, vp, i64, vp,
                                           ctypes.POINTER(Stats)]
    lib.rlap_approx_chol_from_edges.restype = ci
    lib.rlap_approx_chol_from_edges.argtypes = [vp, vp, vp, vp, i64, i64, i64, ctypes.c_double, ci, ci, ci, vp, u64, vp, i64,
                                                ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(Stats)]
    lib.rlap_debug_set_limits.restype = ci
    lib.rlap_debug_set_limits.argtypes = [vp, ctypes.c_double, ctypes.c_double, i64, i64]
    lib.rlap_debug_set_flow_limits.restype = ci
    lib.rlap_debug_set_flow_limits.argtypes = [vp, i64]
    lib.rlap_pack_rows.restype = ci
    lib.rlap_pack_rows.argtypes = [vp, vp, i64, vp]
    lib.rlap_unpack_rows.restype = ci
    lib.rlap_unpack_rows.argtypes = [vp, vp, i64, vp]
    lib.rlap_rng_uniforms.restype = ci
    lib.rlap_rng_uniforms.argtypes = [vp, i64, vp]
    lib.rlap_set_rng_mode.restype = ci
    lib.rlap_set_rng_mode.argtypes = [vp, ci]
    lib.rlap_debug_wave_sort.restype = ci
    lib.rlap_debug_wave_sort.argtypes = [vp, vp, vp, ctypes.c_int32, ctypes.c_int32, vp]
    sz = ctypes.c_size_t
    lib.rlap_workspace_bytes.restype = ci
    lib.rlap_workspace_bytes.argtypes = [i64, i64, i64, ci, ctypes.POINTER(sz), ctypes.POINTER(i64)]
    lib.rlap_workspace_query.restype = ci
    lib.rlap_workspace_query.argtypes = [vp, i64, i64, i64, ci, ctypes.POINTER(sz), ctypes.POINTER(i64)]
    lib.rlap_set_workspace.restype = ci
    lib.rlap_set_workspace.argtypes = [vp, vp, sz, vp, i64]
    lib.rlap_workspace_needed.restype = ci
    lib.rlap_workspace_needed.argtypes = [vp, ctypes.POINTER(sz), ctypes.POINTER(i64)]
    lib.rlap_debug_set_jitter.restype = ci
    lib.rlap_debug_set_jitter.argtypes = [vp, ci]
    lib.rlap_debug_set_poison.restype = ci
    lib.rlap_debug_set_poison.argtypes = [vp, ci]
    lib.rlap_util_ba_graph.restype = i64
    lib.rlap_util_ba_graph.argtypes = [i64, i64, u64, vp, vp]
    _lib = lib
    return lib


def status_string(code):
    return load().rlap_status_string(int(code)).decode()
