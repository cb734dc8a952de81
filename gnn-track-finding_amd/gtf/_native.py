"""ctypes binding of libgtf.so (the C-ABI declared in include/gtf.h).

The library is built in-tree (``__graft_entry__.build()`` / ``make -C
gnn-track-finding_amd/csrc``) and loaded from this directory. There is no CPU
fallback: if the library is missing or fails to load, every call raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GTF_LIB") or os.path.join(HERE, "libgtf.so")   # GTF_LIB: an alternative build

P = ctypes.c_void_p
I32 = ctypes.c_int32
F64 = ctypes.c_double


U32 = ctypes.c_uint32
ABI_VERSION = 8   # GTF_ABI_VERSION of include/gtf.h


class GtfGraph(ctypes.Structure):
    """gtf_graph; keyword construction only -- struct_size / abi_version are filled in,
    and the library refuses a struct of another layout (status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("n_nodes", I32), ("n_slots", I32), ("n_edges", I32), ("n_big", I32),
                ("slot_ptr", P), ("slot_src", P), ("slot_dst", P), ("out_ptr", P), ("out_slot", P),
                ("slot_outpos", P),
                ("is_edge", P), ("rev_edge", P), ("solo", P), ("gnn", P), ("xyzr", P), ("layer", P),
                ("sched", P), ("n_g8", I32), ("n_g16", I32), ("n_g32", I32), ("n_g64", I32), ("out_dst", P),
                ("slot_layer", P), ("n_g4", I32), ("sched_seg", P),
                ("out_sched", P), ("n_o4", I32), ("n_o8", I32), ("n_o16", I32), ("n_g2", I32),
                ("pack_ent", P), ("pack_wave", P), ("n_pack_waves", I32), ("out_lanes", P),
                ("pad_tiles", I32), ("pad_tile_nodes", I32), ("pad_tile_slots", I32), ("pad_count", I32 * 6),
                ("pad_reserved_", I32), ("slot_outidx", P), ("slot_class", P), ("slot_sflags", P),
                ("slot_sxzr", P), ("slot_static", P), ("slot_xclass", P), ("n_g6", I32), ("n_g12", I32)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfGraph)
        self.abi_version = ABI_VERSION


class GtfGraphTables(ctypes.Structure):
    """gtf_graph_tables: the caller-allocated outputs of gtf_graph_prepare (NULL = not wanted)"""
    _fields_ = [("slot_dst", P), ("out_dst", P), ("slot_layer", P), ("slot_outpos", P), ("slot_outidx", P),
                ("slot_class", P), ("slot_sflags", P), ("slot_xclass", P), ("slot_sxzr", P), ("slot_static", P),
                ("sched", P), ("sched_seg", P), ("out_sched", P), ("out_lanes", P)]


class GtfSubsetCounts(ctypes.Structure):
    """gtf_subset_counts: the sizes gtf_graph_subset_plan found for the result"""
    _fields_ = [("n_nodes", I32), ("n_slots", I32), ("n_edges", I32), ("n_sub", I32)]


class GtfSubsetOut(ctypes.Structure):
    """gtf_subset_out: the caller-allocated outputs of gtf_graph_subset_apply (NULL = not wanted)"""
    _fields_ = [("node_map", P), ("slot_map", P), ("slot_ptr", P), ("slot_src", P), ("out_ptr", P),
                ("out_slot", P), ("sub_id", P), ("solo", P)]


class GtfColumn(ctypes.Structure):
    """gtf_column: one column of gtf_subset_gather"""
    _fields_ = [("src", P), ("dst", P), ("row_bytes", I32), ("fill", I32)]


COL_COPY, COL_ZERO_ORPHAN, COL_NAN_ORPHAN, COL_ZERO_ALL = 0, 1, 2, 3   # GTF_COL_*


class GtfNodes(ctypes.Structure):
    _fields_ = [("has_merged", P), ("merged_state", P), ("merged_cov", P), ("merged_prior", P),
                ("has_tse", P), ("has_uts", P), ("degree", P)]


class GtfStates(ctypes.Structure):
    _fields_ = [("rank", P), ("sv", P), ("tau", P), ("cov", P), ("xyzr", P), ("lik", P), ("mw", P),
                ("prior", P), ("lr", P), ("side", P), ("fresh", P)]


class GtfEdges(ctypes.Structure):
    _fields_ = [("act", P), ("edge_mw", P), ("send_mw", P)]


class GtfParams(ctypes.Structure):
    _fields_ = [("sigma0xy", F64), ("sigma0rz", F64), ("sigma0rz2", F64), ("endcap_boundary", F64),
                ("chi2_cut", F64), ("reweight_threshold", F64), ("cluster_chi2", F64), ("cluster_kl", F64)]


class GtfShard(ctypes.Structure):
    _fields_ = [("senders", P), ("n_senders", I32), ("node_lo", I32), ("node_hi", I32), ("slot_lo", I32),
                ("slot_hi", I32), ("phases", I32), ("slot_list", P), ("n_slot_list", I32), ("pad_", I32)]


class GtfHalo(ctypes.Structure):
    _fields_ = [("node_idx", P), ("node_off", P), ("n_nodes", I32), ("pad_", I32), ("slot_idx", P), ("slot_off", P),
                ("n_slots", I32), ("pad2_", I32)]


HALO_NODE_BYTES = 80   # GTF_HALO_NODE_BYTES


class GtfTseExtra(ctypes.Structure):
    _fields_ = [("theta", P), ("var_ms", P), ("xy_mean_var", P), ("zr_mean_var", P), ("angle", P),
                ("translation", P)]


class GtfExtractParams(ctypes.Structure):
    _fields_ = [("p_accept", F64), ("fragment", I32), ("pad_", I32), ("separation_3d", F64),
                ("merge_distance", F64), ("sigma0xy", F64), ("sigma0rz", F64), ("endcap_boundary", F64)]


class GtfExtractIO(ctypes.Structure):
    _fields_ = [("xyzr", P), ("vivl", P), ("sub_id", P), ("sub_ptr", P), ("n_sub", I32), ("pad_", I32),
                ("order_key", P), ("gnn", P), ("label", P), ("status", P), ("pval_xy", P), ("pval_zr", P),
                ("extracted", P), ("n_candidates", P)]


class GtfOrderCounts(ctypes.Structure):
    """gtf_order_counts: what gtf_candidate_order_device met"""
    _fields_ = [("n_components", I32), ("n_set_ordered", I32), ("max_set_ordered", I32), ("pad_", I32)]


class GtfExtractOut(ctypes.Structure):
    """gtf_extract_out: the caller-allocated outputs of gtf_extract_outputs (NULL = not wanted)"""
    _fields_ = [("left", P), ("keep", P), ("cand_ptr", P), ("cand_members", P), ("pval_xy", P), ("pval_zr", P),
                ("rem_ptr", P), ("rem_nodes", P), ("frag_ptr", P), ("frag_nodes", P), ("node_id", P),
                ("cand_ids", P), ("rem_ids", P), ("frag_ids", P)]


class GtfExtractOutCounts(ctypes.Structure):
    _fields_ = [("n_extracted", I32), ("n_extracted_nodes", I32), ("n_remaining", I32), ("n_remaining_nodes", I32),
                ("n_fragments", I32), ("n_fragment_nodes", I32)]


class GtfTruth(ctypes.Structure):
    """gtf_truth: the event's truth tables on the device; keyword construction only --
    struct_size / abi_version are filled in (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("n_nodes", I32), ("n_entries", I32),
                ("n_particles", I32), ("pad_", I32), ("node_id", P), ("node_ptr", P), ("node_part", P),
                ("part_id", P), ("part_hits", P), ("part_ref", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfTruth)
        self.abi_version = ABI_VERSION


class GtfScoreState(ctypes.Structure):
    """gtf_score_state: the per-particle claims the scoring calls accumulate"""
    _fields_ = [("n_particles", I32), ("pad_", I32), ("best_key", P), ("best_good", P), ("best_total", P),
                ("error", P)]


class GtfScoreOut(ctypes.Structure):
    """gtf_score_out: optional per-candidate results of gtf_score_candidates (NULL = not wanted)"""
    _fields_ = [("pid", P), ("n_good", P), ("total", P), ("passes", P)]


class GtfScoreCounts(ctypes.Structure):
    _fields_ = [("n_reconstructed", I32), ("error", U32)]


SCORE_ERR_MISSING, SCORE_ERR_WORKSPACE, SCORE_ERR_RANGE = 1, 2, 4   # GTF_SCORE_ERR_*


class GtfTruthBatch(ctypes.Structure):
    """gtf_truth_batch: K events' truth tables end to end on the device; keyword construction only --
    struct_size / abi_version are filled in (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("n_events", I32), ("n_nodes", I32), ("n_entries", I32),
                ("n_particles", I32), ("node_off", P), ("entry_off", P), ("part_off", P), ("node_id", P),
                ("node_ptr", P), ("node_part", P), ("part_id", P), ("part_hits", P), ("part_ref", P), ("scored", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfTruthBatch)
        self.abi_version = ABI_VERSION


class GtfTruthSizes(ctypes.Structure):
    """gtf_truth_sizes: the sizes of one part of gtf_truth_concat (a host array)"""
    _fields_ = [("n_nodes", I32), ("n_entries", I32), ("n_particles", I32), ("pad_", I32)]


class GtfTruthPart(ctypes.Structure):
    """gtf_truth_part: one entry of gtf_truth_concat's device table"""
    _fields_ = [("n_nodes", I32), ("n_entries", I32), ("n_particles", I32), ("pad_", I32), ("node_id", P),
                ("node_ptr", P), ("node_part", P), ("part_id", P), ("part_hits", P), ("part_ref", P)]


class GtfTruthBatchBuf(ctypes.Structure):
    """gtf_truth_batch_buf: the caller-allocated outputs of gtf_truth_concat"""
    _fields_ = [("node_off", P), ("entry_off", P), ("part_off", P), ("node_id", P), ("node_ptr", P),
                ("node_part", P), ("part_id", P), ("part_hits", P), ("part_ref", P)]


class GtfScoreStateEv(ctypes.Structure):
    """gtf_score_state_ev: the per-particle claims of a whole batch; keyword construction only --
    struct_size / abi_version are filled in (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("n_particles", I32), ("pad_", I32), ("best_key", P),
                ("best_good", P), ("best_total", P), ("error", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfScoreStateEv)
        self.abi_version = ABI_VERSION


class GtfTruthIn(ctypes.Structure):
    """gtf_truth_in: the parsed columns gtf_truth_build reads, device arrays; keyword construction
    only -- struct_size / abi_version are filled in (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("n_rows", I32), ("n_truth", I32),
                ("n_particles", I32), ("num_layers", I32), ("min_volume", I32), ("max_volume", I32),
                ("pt_cut", F64), ("node_idx", P), ("hit_id", P), ("particle_id", P), ("volume_id", P),
                ("layer_id", P), ("module_id", P), ("truth_hit", P), ("truth_part", P), ("part_id", P),
                ("px", P), ("py", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfTruthIn)
        self.abi_version = ABI_VERSION


class GtfTruthBuf(ctypes.Structure):
    """gtf_truth_buf: the caller-allocated outputs of gtf_truth_build, each at its bound n_rows (+ 1)"""
    _fields_ = [("node_id", P), ("node_ptr", P), ("node_part", P), ("part_id", P), ("part_hits", P),
                ("part_ref", P)]


class GtfTruthCounts(ctypes.Structure):
    _fields_ = [("n_nodes", I32), ("n_entries", I32), ("n_particles", I32), ("n_reference", I32),
                ("error", U32), ("pad_", I32)]


class GtfTruthInEv(ctypes.Structure):
    """gtf_truth_in_ev: the parsed columns of K events end to end that gtf_truth_build_ev reads: three
    HOST offset arrays [K + 1] and eleven device columns; keyword construction only -- struct_size /
    abi_version are filled in (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("n_events", I32), ("num_layers", I32),
                ("min_volume", I32), ("max_volume", I32), ("pt_cut", F64), ("row_off", P), ("truth_off", P),
                ("particle_off", P), ("node_idx", P), ("hit_id", P), ("particle_id", P), ("volume_id", P),
                ("layer_id", P), ("module_id", P), ("truth_hit", P), ("truth_part", P), ("part_id", P),
                ("px", P), ("py", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfTruthInEv)
        self.abi_version = ABI_VERSION


TRUTH_ERR_MISSING, TRUTH_ERR_RANGE = 1, 2   # GTF_TRUTH_ERR_*
TRUTH_ID_LIMIT = 1 << 21                    # volume_id, layer_id, module_id: [0, 2^21)


class GtfEventCsr(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_int64), ("n_rows", ctypes.c_int64), ("node_id", P), ("row_a", P),
                ("row_b", P), ("order", P), ("sub_id", P), ("slot_ptr", P), ("slot_src", P), ("tse_rank", P),
                ("out_ptr", P), ("out_slot", P), ("n_edges", ctypes.c_int64), ("n_subgraphs", I32), ("pad_", I32)]


class GtfEventBatch(ctypes.Structure):
    """gtf_event_batch: the events of gtf_build_events_csr_device (node_off / row_off: HOST int32 [K + 1];
    event: a device int32 [N] or NULL); keyword construction only -- struct_size / abi_version are filled in
    (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("n_events", I32), ("pad_", I32), ("node_off", P),
                ("row_off", P), ("event", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfEventBatch)
        self.abi_version = ABI_VERSION


class GtfEventCols(ctypes.Structure):
    """gtf_event_cols: the CSV columns of the kept nodes, device arrays in CSV row order"""
    _fields_ = [("x", P), ("y", P), ("z", P), ("r", P), ("layer_id", P)]


class GtfEventOut(ctypes.Structure):
    """gtf_event_out: the caller-allocated outputs of gtf_event_pack (NULL = not wanted)"""
    _fields_ = [("gnn", P), ("xyzr", P), ("layer", P), ("node_id", P), ("vivl", P), ("solo", P)]


class GtfFillColumn(ctypes.Structure):
    """gtf_fill_column: one column of gtf_fill_columns"""
    _fields_ = [("dst", P), ("rows", ctypes.c_int64), ("row_bytes", I32), ("pad_", I32),
                ("pattern", ctypes.c_uint64)]


FILL_MAX_COLUMNS = 32   # GTF_FILL_MAX_COLUMNS


class GtfConcatSizes(ctypes.Structure):
    """gtf_concat_sizes: the sizes of one part of gtf_graph_concat (a host array)"""
    _fields_ = [("n_nodes", I32), ("n_slots", I32), ("n_edges", I32), ("n_sub", I32)]


class GtfConcatPart(ctypes.Structure):
    """gtf_concat_part: one entry of gtf_graph_concat's device table"""
    _fields_ = [("n_nodes", I32), ("n_slots", I32), ("n_edges", I32), ("n_sub", I32), ("slot_ptr", P),
                ("slot_src", P), ("out_ptr", P), ("out_slot", P), ("sub_id", P)]


class GtfConcatOut(ctypes.Structure):
    """gtf_concat_out: the structure arrays of the fused graph (NULL = not wanted); keyword construction
    only -- struct_size / abi_version are filled in (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("slot_ptr", P), ("slot_src", P), ("out_ptr", P),
                ("out_slot", P), ("sub_id", P), ("event", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfConcatOut)
        self.abi_version = ABI_VERSION


class GtfConcatColumn(ctypes.Structure):
    """gtf_concat_column: one payload column of gtf_concat_columns (src: a device table of n_parts pointers)"""
    _fields_ = [("src", P), ("dst", P), ("row_bytes", I32), ("axis", I32)]


CONCAT_MAX_COLUMNS = 32   # GTF_CONCAT_MAX_COLUMNS


class GtfSplitIn(ctypes.Structure):
    """gtf_split_in: the lists of one gtf_extract_outputs call, as node indices; keyword construction
    only -- struct_size / abi_version are filled in (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("cand_ptr", P), ("cand_members", P), ("rem_ptr", P),
                ("rem_nodes", P), ("frag_ptr", P), ("frag_nodes", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfSplitIn)
        self.abi_version = ABI_VERSION


class GtfSplitOut(ctypes.Structure):
    """gtf_split_out: gtf_event_split's device outputs"""
    _fields_ = [("cand_first", P), ("rem_first", P), ("frag_first", P), ("counts", P), ("cand_ptr_ev", P)]


class GtfEventErrorsIo(ctypes.Structure):
    """gtf_event_errors_io: node_err per event; keyword construction only -- struct_size / abi_version
    are filled in (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("node_err", P), ("event", P), ("node_id", P),
                ("n_nodes", I32), ("n_events", I32), ("mask", U32), ("pad_", U32), ("err_ev", P), ("n_raising", P),
                ("first_node", P), ("first_id", P), ("keep", P), ("host_err_ev", P), ("host_n_raising", P),
                ("host_first_node", P), ("host_first_id", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfEventErrorsIo)
        self.abi_version = ABI_VERSION


CSV_MAX_COLUMNS, CSV_MAX_FIELDS, CSV_MAX_ROW_BYTES = 16, 64, 1024   # GTF_CSV_MAX_*
CSV_INT64, CSV_DOUBLE = 0, 1                                        # GTF_CSV_INT64 / _DOUBLE
# GTF_CSV_ERR_*
(CSV_ERR_DIGITS, CSV_ERR_EXPONENT, CSV_ERR_TEXT, CSV_ERR_EMPTY, CSV_ERR_QUOTE, CSV_ERR_SPACE, CSV_ERR_INT_FORM,
 CSV_ERR_FIELDS, CSV_ERR_ROW_LONG, CSV_ERR_ROWS) = (1 << k for k in range(10))
CSV_ERRORS = {CSV_ERR_DIGITS: "more digits than the exact domain holds", CSV_ERR_EXPONENT: "decimal exponent beyond 22",
              CSV_ERR_TEXT: "not a number", CSV_ERR_EMPTY: "empty field", CSV_ERR_QUOTE: "quoted field",
              CSV_ERR_SPACE: "space or tab inside a field", CSV_ERR_INT_FORM: "point or exponent in an integer column",
              CSV_ERR_FIELDS: "wrong number of fields", CSV_ERR_ROW_LONG: "row longer than 1024 bytes",
              CSV_ERR_ROWS: "more rows than max_rows"}


class GtfCsvColumn(ctypes.Structure):
    """gtf_csv_column: one requested field of gtf_csv_parse"""
    _fields_ = [("field", I32), ("type", I32), ("out", P)]


class GtfCsvIn(ctypes.Structure):
    """gtf_csv_in; keyword construction only -- struct_size / abi_version are filled in"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("text", P), ("n_bytes", I32), ("skip_lines", I32),
                ("n_fields", I32), ("max_rows", I32), ("n_columns", I32), ("delimiter", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8 * 3), ("columns", GtfCsvColumn * CSV_MAX_COLUMNS)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfCsvIn)
        self.abi_version = ABI_VERSION


class GtfCsvCounts(ctypes.Structure):
    _fields_ = [("n_rows", I32), ("error", U32), ("first_bad_row", I32), ("first_bad_field", I32),
                ("first_bad_error", U32), ("pad_", I32)]


class GtfCsvFile(ctypes.Structure):
    """gtf_csv_file: one file of gtf_csv_parse_ev's host table"""
    _fields_ = [("start", I32), ("n_bytes", I32)]


class GtfCsvInEv(ctypes.Structure):
    """gtf_csv_in_ev; keyword construction only -- struct_size / abi_version are filled in"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("text", P), ("files", P), ("row_off", P),
                ("n_files", I32), ("skip_lines", I32), ("n_fields", I32), ("max_rows", I32), ("n_columns", I32),
                ("delimiter", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 3),
                ("columns", GtfCsvColumn * CSV_MAX_COLUMNS)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfCsvInEv)
        self.abi_version = ABI_VERSION


class GtfWindowIn(ctypes.Structure):
    """gtf_window_in; keyword construction only -- struct_size / abi_version are filled in"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("n_rows", I32), ("pad_", I32), ("lo", ctypes.c_int64),
                ("hi", ctypes.c_int64), ("node_idx", P), ("layer_id", P), ("x", P), ("y", P), ("z", P)]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.struct_size = ctypes.sizeof(GtfWindowIn)
        self.abi_version = ABI_VERSION


class GtfWindowOut(ctypes.Structure):
    """gtf_window_out: the caller-allocated outputs of gtf_event_window, each [n_rows]"""
    _fields_ = [("node_idx", P), ("layer_id", P), ("x", P), ("y", P), ("z", P), ("r", P), ("amb_index", P),
                ("amb_x", P), ("amb_y", P)]


class GtfWindowCounts(ctypes.Structure):
    _fields_ = [("n_kept", I32), ("n_ambiguous", I32)]


class GtfCandidateGraph(ctypes.Structure):
    _fields_ = [("n_nodes", I32), ("n_slots", I32), ("n_edges", I32), ("pad_", I32), ("slot_ptr", P),
                ("slot_src", P), ("is_edge", P), ("act", P), ("out_ptr", P), ("out_slot", P), ("sub_id", P),
                ("node_id", P)]


class GtfKlGraph(ctypes.Structure):
    _fields_ = [("n_nodes", I32), ("n_slots", I32), ("slot_ptr", P), ("slot_src", P), ("gnn", P), ("truth", P),
                ("pair_ptr", P), ("list", P * 4), ("count", I32 * 4), ("first", I32 * 4), ("n_d1", I32),
                ("gnn_stride", I32), ("slot0", ctypes.c_int64), ("pair0", ctypes.c_int64), ("blk", P),
                ("n_blk", I32), ("deg_runs", I32), ("n_deg", I32 * 6), ("pad_deg_", I32)]


class GtfDiag(ctypes.Structure):
    _fields_ = [("node_err", P), ("edge_chi2", P), ("slot_cluster", P), ("reserved_", P * 5)]


DIAG_OFFSET = 64
COMM_ID_BYTES = 128   # GTF_COMM_ID_BYTES


class GtfPairOut(ctypes.Structure):
    _fields_ = [("chi2", P), ("avg_tau", P), ("avg_theta", P), ("delta_theta", P), ("truth", P), ("err", P)]


class GtfKlOut(ctypes.Structure):
    _fields_ = [("kl", P), ("truth", P), ("emp_var", P), ("emp_mean", P), ("sv", P), ("cov", P), ("err", P)]


class GtfKlQ32(ctypes.Structure):
    _fields_ = [("xy", P), ("scale", ctypes.c_double), ("truth32", P)]


class GtfKlOut32(ctypes.Structure):
    _fields_ = [("kl", P), ("truth", P), ("emp_var", P), ("emp_mean", P), ("err", P)]


class GtfKlPrepareIn(ctypes.Structure):
    """gtf_kl_prepare_in: what gtf_kl_prepare reads, device arrays; keyword construction only --
    struct_size / abi_version are filled in (another layout: status -3)"""
    _fields_ = [("struct_size", U32), ("abi_version", U32), ("n_nodes", I32), ("n_slots", I32), ("slot_ptr", P),
                ("slot_src", P), ("is_edge", P), ("gnn", P), ("truth", P), ("gnn_stride", I32), ("with_single", I32),
                ("layout", I32), ("compact", I32), ("scale", ctypes.c_double)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(GtfKlPrepareIn)
        self.abi_version = ABI_VERSION


class GtfKlPrepareBuf(ctypes.Structure):
    """gtf_kl_prepare_buf: the caller-allocated outputs of gtf_kl_prepare"""
    _fields_ = [("slot_ptr", P), ("slot_src", P), ("xy", P), ("truth", P), ("pair_ptr", P), ("list", P),
                ("node_of", P), ("slot_of", P), ("q", P), ("truth32", P)]


class GtfKlCounts(ctypes.Structure):
    _fields_ = [("n_kept", I32), ("n_listed", I32), ("n_pairs", ctypes.c_int64), ("count", I32 * 4),
                ("first", I32 * 4), ("n_d1", I32), ("n_deg", I32 * 6), ("error", U32), ("scale", ctypes.c_double),
                ("max_abs", ctypes.c_double)]


KL_ERR_SLOT_PTR, KL_ERR_SOURCE, KL_ERR_NONFINITE, KL_ERR_FIT, KL_ERR_SCALE, KL_ERR_NODE_OF = 1, 2, 4, 8, 16, 32


GTF_F64, GTF_F32 = 0, 1

ERR_FLAGS = {
    1: "KeyError: sender has no track_state_estimates entry for the receiver (extrapolate_merged_states.py:384)",
    2: "KeyError: last state key has no edge (helper.py:131/138)",
    4: "ValueError: all pairwise distances are zero (clustering.py:120)",
    8: "ValueError: a distance tie removed every state (clustering.py:116)",
    16: "ZeroDivisionError: empty state dict (helper.py:90)",
    32: "ValueError: NaN KL distance (clustering.py:117)",
    64: "KeyError: node has no state dict (remove_state_metadata.py:39)",
    128: "LinAlgError: singular parabola matrix H (helper.py:384; learn_KL_parabolic_model utils.py:277)",
    256: "pair_ptr disagrees with the updated_track_states dicts (caller error)",
    512: "KeyError: neighbour not in the subgraph (calculate_distance_between_updated_track_states.py:182-183)",
    1024: "a node holds more than 2048 updated track states (not processed)",
}

# exported symbols (must match include/gtf.h; tests check the .so exports all of them)
SYMBOLS = ["gtf_workspace_bytes", "gtf_workspace_init", "gtf_uts_materialize", "gtf_clear_errors", "gtf_read_errors", "gtf_extrapolate", "gtf_update",
           "gtf_message_passing", "gtf_node_ops",
           "gtf_cluster", "gtf_pass", "gtf_pass_ev", "gtf_tag_prepare", "gtf_tag_sweep", "gtf_tag_sweep_shard", "gtf_tag_workspace_bytes", "gtf_tag_propagate", "gtf_parabolic_kl", "gtf_parabolic_kl_q32", "gtf_track_state_estimates", "gtf_track_state_estimates_ws", "gtf_pass_shard",
           "gtf_shard_chunk_bytes", "gtf_shard_pack", "gtf_shard_unpack", "gtf_halo_pack", "gtf_halo_unpack",
           "gtf_extract_workspace_bytes",
           "gtf_extract_candidates", "gtf_build_event_csr", "gtf_candidate_order",
           "gtf_subgraph_ptr_device", "gtf_candidate_order_workspace_bytes", "gtf_candidate_order_device",
           "gtf_candidate_order_device_ev",
           "gtf_graph_concat_workspace_bytes", "gtf_graph_concat", "gtf_concat_columns",
           "gtf_event_split_workspace_bytes", "gtf_event_split",
           "gtf_event_errors_workspace_bytes", "gtf_event_errors",
           "gtf_extract_outputs_workspace_bytes", "gtf_extract_outputs",
           "gtf_score_reset", "gtf_score_workspace_bytes", "gtf_score_candidates",
           "gtf_score_finish_workspace_bytes", "gtf_score_finish",
           "gtf_truth_concat_workspace_bytes", "gtf_truth_concat", "gtf_score_reset_ev",
           "gtf_score_ev_workspace_bytes", "gtf_score_candidates_ev",
           "gtf_score_finish_ev_workspace_bytes", "gtf_score_finish_ev",
           "gtf_truth_build_workspace_bytes", "gtf_truth_build",
           "gtf_truth_build_ev_workspace_bytes", "gtf_truth_build_ev",
           "gtf_kl_prepare_workspace_bytes", "gtf_kl_prepare", "gtf_kl_coords", "gtf_kl_pair_rows",
           "gtf_build_event_device_workspace_bytes", "gtf_build_event_csr_device",
           "gtf_build_events_device_workspace_bytes", "gtf_build_events_csr_device",
           "gtf_graph_prepare_workspace_bytes", "gtf_graph_prepare",
           "gtf_graph_subset_workspace_bytes", "gtf_graph_subset_plan", "gtf_graph_subset_apply",
           "gtf_subset_gather", "gtf_refresh_send_mw", "gtf_event_pack", "gtf_fill_columns",
           "gtf_csv_chunk_bytes", "gtf_csv_parse_workspace_bytes", "gtf_csv_parse",
           "gtf_csv_parse_ev_workspace_bytes", "gtf_csv_parse_ev",
           "gtf_event_window_workspace_bytes", "gtf_event_window", "gtf_event_radius_patch",
           "gtf_event_window_ev_workspace_bytes", "gtf_event_window_ev",
           "gtf_updated_state_pair_counts", "gtf_updated_state_distances", "gtf_set_diagnostics",
           "gtf_device_init", "gtf_malloc", "gtf_free", "gtf_memcpy_htod", "gtf_memcpy_dtoh", "gtf_memcpy_dtod",
           "gtf_memset", "gtf_stream_synchronize",
           "gtf_comm_unique_id", "gtf_comm_init", "gtf_comm_destroy", "gtf_comm_rank", "gtf_comm_size",
           "gtf_halo_exchange", "gtf_halo_alltoall", "gtf_allreduce_max_i64", "gtf_allgather_bytes",
           "gtf_tag_shard_workspace_bytes",
           "gtf_tag_propagate_shard",
           "gtf_last_error",
           "gtf_version"]

OPS = {"ranks": 1, "priors_tse": 2, "priors_uts": 3, "reweight_uts": 4, "degree": 5, "prune": 6, "mw_tse": 7,
       "mw_uts": 8, "cluster_tse": 9, "cluster_uts": 10, "fresh": 11}

_lib = None
_lean = False   # loaded without torch (lean=True): only gtf.devmem allocations may be used


def lib(lean: bool = False):
    """Load libgtf.so once; raise loudly if it is missing (no fallback path).

    lean=False (default): torch is imported first, so its bundled libamdhip64 (SONAME
    libamdhip64.so.7) satisfies libgtf's NEEDED entry and the process holds ONE HIP
    runtime, which torch tensors and libgtf share. Loaded the other way round, torch
    pulls a second runtime and libgtf's calls see no device.
    lean=True (the drop-in CLIs, gtf.devmem): torch is not imported; libgtf binds the
    system HIP runtime and every allocation comes from gtf_malloc. A process that loaded
    libgtf this way cannot use torch device tensors with it afterwards (lib() raises)."""
    global _lib, _lean
    if _lib is not None:
        if _lean and not lean:
            raise RuntimeError("libgtf was loaded without torch (gtf.devmem, the drop-in CLIs' lean runtime); "
                               "torch device tensors cannot share it in this process")
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libgtf.so not built at %s -- run __graft_entry__.build() "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    import sys
    if lean and "torch" not in sys.modules:
        _lean = True
    else:
        import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    L.gtf_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_workspace_bytes.argtypes = [I32, I32]
    L.gtf_clear_errors.argtypes = [P, P]
    L.gtf_workspace_init.argtypes = [P, P]
    L.gtf_read_errors.argtypes = [P, ctypes.POINTER(ctypes.c_uint32), P]
    L.gtf_set_diagnostics.argtypes = [P, ctypes.POINTER(GtfDiag), P]
    G, N, S, E, PR = (ctypes.POINTER(GtfGraph), ctypes.POINTER(GtfNodes), ctypes.POINTER(GtfStates),
                      ctypes.POINTER(GtfEdges), ctypes.POINTER(GtfParams))
    L.gtf_extrapolate.argtypes = [G, N, S, E, PR, P, P]
    L.gtf_uts_materialize.argtypes = [G, S, P]
    L.gtf_update.argtypes = [G, N, S, S, E, PR, P, P]
    L.gtf_message_passing.argtypes = [G, N, S, E, PR, P, P]
    L.gtf_node_ops.argtypes = [G, N, S, S, E, PR, ctypes.POINTER(ctypes.c_int8), I32, F64, F64, P, P]
    L.gtf_cluster.argtypes = [G, N, S, E, I32, F64, F64, PR, P, P]
    L.gtf_pass.argtypes = [G, N, S, S, E, PR, P, P]
    L.gtf_pass_ev.argtypes = [G, N, S, S, E, PR, P, P, ctypes.POINTER(P)]
    L.gtf_tag_prepare.argtypes = [G, P, P, P, P, P]
    L.gtf_tag_sweep.argtypes = [G, P, P, P, P, P, P]
    L.gtf_tag_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_tag_workspace_bytes.argtypes = [I32, I32]
    L.gtf_tag_propagate.argtypes = [G, P, P, F64, I32, P, ctypes.POINTER(ctypes.c_int32), P, ctypes.c_size_t, P]
    L.gtf_extract_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_extract_workspace_bytes.argtypes = [I32, I32]
    L.gtf_extract_candidates.argtypes = [G, E, ctypes.POINTER(GtfExtractIO), ctypes.POINTER(GtfExtractParams), P, P]
    L.gtf_subgraph_ptr_device.argtypes = [P, I32, I32, P, P]
    L.gtf_candidate_order_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_candidate_order_workspace_bytes.argtypes = [I32, I32, I32]
    L.gtf_candidate_order_device.argtypes = [G, E, P, P, I32, P, P, P, ctypes.c_size_t,
                                             ctypes.POINTER(GtfOrderCounts), P]
    L.gtf_candidate_order_device_ev.argtypes = [G, E, P, P, I32, P, P, P, P, ctypes.c_size_t,
                                                ctypes.POINTER(GtfOrderCounts), P]
    L.gtf_graph_concat_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_graph_concat_workspace_bytes.argtypes = [I32]
    L.gtf_graph_concat.argtypes = [ctypes.POINTER(GtfConcatSizes), P, I32, ctypes.POINTER(GtfConcatOut), P,
                                   ctypes.c_size_t, P]
    L.gtf_concat_columns.argtypes = [P, I32, I32, I32, ctypes.POINTER(GtfConcatColumn), I32, P]
    L.gtf_event_split_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_event_split_workspace_bytes.argtypes = [I32]
    L.gtf_event_split.argtypes = [P, I32, I32, ctypes.POINTER(GtfExtractOutCounts), ctypes.POINTER(GtfSplitIn),
                                  ctypes.POINTER(GtfSplitOut), P, ctypes.c_size_t, P]
    L.gtf_event_errors_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_event_errors_workspace_bytes.argtypes = [I32]
    L.gtf_event_errors.argtypes = [ctypes.POINTER(GtfEventErrorsIo), P, ctypes.c_size_t, P]
    L.gtf_extract_outputs_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_extract_outputs_workspace_bytes.argtypes = [I32, I32]
    L.gtf_extract_outputs.argtypes = [G, ctypes.POINTER(GtfExtractIO), I32, P, ctypes.POINTER(GtfExtractOut), P,
                                      ctypes.c_size_t, ctypes.POINTER(GtfExtractOutCounts), P]
    TR, SS = ctypes.POINTER(GtfTruth), ctypes.POINTER(GtfScoreState)
    L.gtf_score_reset.argtypes = [SS, P]
    L.gtf_score_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_score_workspace_bytes.argtypes = [I32, I32]
    L.gtf_score_candidates.argtypes = [TR, P, P, I32, I32, ctypes.POINTER(GtfScoreOut), SS, P, ctypes.c_size_t, P]
    L.gtf_score_finish_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_score_finish_workspace_bytes.argtypes = [I32]
    L.gtf_score_finish.argtypes = [TR, SS, P, P, P, P, P, ctypes.POINTER(GtfScoreCounts), P, ctypes.c_size_t, P]
    TB, SE = ctypes.POINTER(GtfTruthBatch), ctypes.POINTER(GtfScoreStateEv)
    L.gtf_truth_concat_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_truth_concat_workspace_bytes.argtypes = [I32]
    L.gtf_truth_concat.argtypes = [ctypes.POINTER(GtfTruthSizes), P, I32, ctypes.POINTER(GtfTruthBatchBuf), TB, P,
                                   ctypes.c_size_t, P]
    L.gtf_score_reset_ev.argtypes = [SE, TB, P, P]
    L.gtf_score_ev_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_score_ev_workspace_bytes.argtypes = [I32, I32, I32]
    L.gtf_score_candidates_ev.argtypes = [TB, P, P, P, I32, I32, ctypes.POINTER(GtfScoreOut), SE, P, ctypes.c_size_t, P]
    L.gtf_score_finish_ev_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_score_finish_ev_workspace_bytes.argtypes = [I32, I32]
    L.gtf_score_finish_ev.argtypes = [TB, SE, P, P, P, P, P, P, P, P, P, ctypes.c_size_t, P]
    L.gtf_truth_build_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_truth_build_workspace_bytes.argtypes = [I32, I32, I32]
    L.gtf_truth_build.argtypes = [ctypes.POINTER(GtfTruthIn), ctypes.POINTER(GtfTruthBuf), TR,
                                  ctypes.POINTER(GtfTruthCounts), P, ctypes.c_size_t, P]
    L.gtf_truth_build_ev_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_truth_build_ev_workspace_bytes.argtypes = [I32, I32, I32, I32]
    L.gtf_truth_build_ev.argtypes = [ctypes.POINTER(GtfTruthInEv), ctypes.POINTER(GtfTruthBatchBuf), TB,
                                     ctypes.POINTER(GtfTruthCounts), P, ctypes.c_size_t, P]
    SH =ctypes.POINTER(GtfShard)
    L.gtf_pass_shard.argtypes = [G, N, S, S, E, PR, SH, P, P, ctypes.POINTER(P)]
    L.gtf_tag_sweep_shard.argtypes = [G, P, P, P, P, SH, I32, I32, P]
    L.gtf_shard_chunk_bytes.restype = ctypes.c_size_t
    L.gtf_shard_chunk_bytes.argtypes = [I32, I32]
    L.gtf_shard_pack.argtypes = [N, E, SH, I32, I32, P, P]
    L.gtf_shard_unpack.argtypes = [N, E, P, I32, I32, P, I32, I32, P]
    HA = ctypes.POINTER(GtfHalo)
    L.gtf_halo_pack.argtypes = [N, E, HA, P, P]
    L.gtf_halo_unpack.argtypes = [N, E, HA, P, P]
    L.gtf_track_state_estimates.argtypes = [G, S, ctypes.POINTER(GtfTseExtra), PR, P]
    L.gtf_track_state_estimates_ws.argtypes = [G, S, ctypes.POINTER(GtfTseExtra), PR, P, P]
    L.gtf_parabolic_kl.argtypes = [ctypes.POINTER(GtfKlGraph), I32, ctypes.POINTER(GtfKlOut), P]
    L.gtf_parabolic_kl_q32.argtypes = [ctypes.POINTER(GtfKlGraph), ctypes.POINTER(GtfKlQ32),
                                       ctypes.POINTER(GtfKlOut32), P]
    L.gtf_kl_prepare_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_kl_prepare_workspace_bytes.argtypes = [I32, I32]
    L.gtf_kl_prepare.argtypes = [ctypes.POINTER(GtfKlPrepareIn), ctypes.POINTER(GtfKlPrepareBuf),
                                 ctypes.POINTER(GtfKlGraph), ctypes.POINTER(GtfKlQ32), ctypes.POINTER(GtfKlCounts), P,
                                 ctypes.c_size_t, P]
    L.gtf_kl_coords.argtypes = [I32, P, I32, P, P, P, F64, P, P]
    L.gtf_kl_pair_rows.argtypes = [ctypes.POINTER(GtfKlGraph), ctypes.c_int64, P, P, I32, P, P, P, P, P]
    L.gtf_build_event_csr.argtypes = [ctypes.POINTER(GtfEventCsr)]
    L.gtf_build_event_device_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_build_event_device_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
    L.gtf_build_event_csr_device.argtypes = [ctypes.POINTER(GtfEventCsr), P, ctypes.c_size_t, P]
    L.gtf_build_events_device_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_build_events_device_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, I32]
    L.gtf_build_events_csr_device.argtypes = [ctypes.POINTER(GtfEventCsr), ctypes.POINTER(GtfEventBatch), P,
                                              ctypes.c_size_t, P]
    L.gtf_graph_prepare_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_graph_prepare_workspace_bytes.argtypes = [I32, I32, I32]
    L.gtf_graph_prepare.argtypes = [G, ctypes.POINTER(GtfGraphTables), P, ctypes.c_size_t, P]
    L.gtf_graph_subset_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_graph_subset_workspace_bytes.argtypes = [I32, I32, I32, I32]
    L.gtf_graph_subset_plan.argtypes = [G, P, P, P, I32, P, P, ctypes.c_size_t, ctypes.POINTER(GtfSubsetCounts), P]
    L.gtf_graph_subset_apply.argtypes = [G, P, ctypes.POINTER(GtfSubsetOut), P]
    L.gtf_subset_gather.argtypes = [P, I32, ctypes.POINTER(GtfColumn), I32, P]
    L.gtf_refresh_send_mw.argtypes = [G, P, P, P, P]
    L.gtf_event_pack.argtypes = [ctypes.POINTER(GtfEventCsr), ctypes.POINTER(GtfEventCols),
                                 ctypes.POINTER(GtfEventOut), P]
    L.gtf_fill_columns.argtypes = [ctypes.POINTER(GtfFillColumn), I32, P]
    L.gtf_csv_chunk_bytes.restype = ctypes.c_size_t
    L.gtf_csv_chunk_bytes.argtypes = []
    L.gtf_csv_parse_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_csv_parse_workspace_bytes.argtypes = [I32]
    L.gtf_csv_parse.argtypes = [ctypes.POINTER(GtfCsvIn), ctypes.POINTER(GtfCsvCounts), P, ctypes.c_size_t, P]
    L.gtf_csv_parse_ev_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_csv_parse_ev_workspace_bytes.argtypes = [ctypes.c_int64, I32]
    L.gtf_csv_parse_ev.argtypes = [ctypes.POINTER(GtfCsvInEv), ctypes.POINTER(GtfCsvCounts), P, ctypes.c_size_t, P]
    L.gtf_event_window_ev_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_event_window_ev_workspace_bytes.argtypes = [I32, I32]
    L.gtf_event_window_ev.argtypes = [ctypes.POINTER(GtfWindowIn), P, I32, ctypes.POINTER(GtfWindowOut), P,
                                      ctypes.POINTER(GtfWindowCounts), P, ctypes.c_size_t, P]
    L.gtf_event_window_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_event_window_workspace_bytes.argtypes = [I32]
    L.gtf_event_window.argtypes = [ctypes.POINTER(GtfWindowIn), ctypes.POINTER(GtfWindowOut),
                                   ctypes.POINTER(GtfWindowCounts), P, ctypes.c_size_t, P]
    L.gtf_event_radius_patch.argtypes = [P, I32, P, P, I32, P]
    L.gtf_candidate_order.argtypes = [ctypes.POINTER(GtfCandidateGraph), P]
    L.gtf_updated_state_pair_counts.argtypes = [G, N, S, E, P, P]
    L.gtf_updated_state_distances.argtypes = [G, N, S, E, P, P, ctypes.POINTER(GtfPairOut), P]
    L.gtf_device_init.argtypes = [I32]
    L.gtf_malloc.argtypes = [ctypes.POINTER(P), ctypes.c_size_t]
    L.gtf_free.argtypes = [P]
    for fn in ("gtf_memcpy_htod", "gtf_memcpy_dtoh", "gtf_memcpy_dtod"):
        getattr(L, fn).argtypes = [P, P, ctypes.c_size_t, P]
    L.gtf_memset.argtypes = [P, I32, ctypes.c_size_t, P]
    L.gtf_stream_synchronize.argtypes = [P]
    I64 = ctypes.c_int64
    L.gtf_comm_unique_id.argtypes = [P]
    L.gtf_comm_init.argtypes = [ctypes.POINTER(P), I32, I32, P]
    L.gtf_comm_destroy.argtypes = [P]
    L.gtf_comm_rank.argtypes = [P]
    L.gtf_comm_size.argtypes = [P]
    L.gtf_halo_exchange.argtypes = [P, N, E, HA, HA, P, P, P, P, P]
    L.gtf_halo_alltoall.argtypes = [P, P, P, P, P, P]
    L.gtf_allreduce_max_i64.argtypes = [P, P, I64, P]
    L.gtf_allgather_bytes.argtypes = [P, P, P, I64, P]
    L.gtf_tag_shard_workspace_bytes.restype = ctypes.c_size_t
    L.gtf_tag_shard_workspace_bytes.argtypes = [I32, I32, I32]
    L.gtf_tag_propagate_shard.argtypes = [P, G, SH, P, P, F64, I32, P, ctypes.POINTER(ctypes.c_int32), P,
                                          ctypes.c_size_t, P]
    L.gtf_last_error.restype = ctypes.c_char_p
    L.gtf_version.restype = ctypes.c_char_p
    for fn in ("gtf_workspace_init", "gtf_uts_materialize", "gtf_clear_errors", "gtf_read_errors", "gtf_extrapolate", "gtf_update", "gtf_cluster", "gtf_pass",
               "gtf_pass_ev", "gtf_message_passing", "gtf_node_ops",
               "gtf_tag_prepare", "gtf_tag_sweep", "gtf_tag_sweep_shard", "gtf_parabolic_kl", "gtf_parabolic_kl_q32", "gtf_track_state_estimates", "gtf_track_state_estimates_ws", "gtf_pass_shard", "gtf_shard_pack",
               "gtf_shard_unpack", "gtf_halo_pack", "gtf_halo_unpack", "gtf_extract_candidates", "gtf_build_event_csr",
               "gtf_candidate_order", "gtf_updated_state_pair_counts", "gtf_updated_state_distances",
               "gtf_set_diagnostics", "gtf_build_event_csr_device", "gtf_device_init", "gtf_malloc", "gtf_free",
               "gtf_memcpy_htod", "gtf_memcpy_dtoh", "gtf_memcpy_dtod", "gtf_memset", "gtf_stream_synchronize",
               "gtf_comm_unique_id", "gtf_comm_init", "gtf_comm_destroy", "gtf_comm_rank", "gtf_comm_size",
               "gtf_halo_exchange", "gtf_halo_alltoall", "gtf_allreduce_max_i64", "gtf_allgather_bytes",
               "gtf_tag_propagate_shard", "gtf_graph_prepare", "gtf_graph_subset_plan", "gtf_graph_subset_apply",
               "gtf_subset_gather", "gtf_refresh_send_mw", "gtf_subgraph_ptr_device", "gtf_candidate_order_device",
               "gtf_extract_outputs", "gtf_event_pack", "gtf_fill_columns", "gtf_score_reset",
               "gtf_score_candidates", "gtf_score_finish", "gtf_truth_build", "gtf_csv_parse", "gtf_event_window",
               "gtf_event_radius_patch", "gtf_candidate_order_device_ev", "gtf_graph_concat", "gtf_concat_columns",
               "gtf_event_split", "gtf_build_events_csr_device", "gtf_truth_concat", "gtf_score_reset_ev",
               "gtf_score_candidates_ev", "gtf_score_finish_ev", "gtf_truth_build_ev", "gtf_csv_parse_ev",
               "gtf_event_window_ev", "gtf_event_errors", "gtf_kl_prepare", "gtf_kl_coords", "gtf_kl_pair_rows"):
        getattr(L, fn).restype = ctypes.c_int
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RuntimeError("libgtf: %s (rc=%d)" % ((_lib or lib()).gtf_last_error().decode(), rc))
