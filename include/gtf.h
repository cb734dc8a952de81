/*
 * gtf.h -- C-ABI of libgtf.so, the MI355X (gfx950) edge-parallel track-finding
 * pass that drops in behind nishalad95/GNN-track-finding's hot path.
 *
 * Every pointer in the structs below is a DEVICE pointer (HBM) owned by the
 * caller; the library keeps no pointer after a call returns and allocates
 * nothing on the hot path (scratch comes from the caller's workspace). All
 * calls are stream-ordered on the hipStream_t passed in (0 = null stream).
 * Return value: 0 = OK, < 0 = error (gtf_last_error() has the message).
 * Reference-semantics exceptions detected on the device (the places where the
 * reference itself raises) are reported as bit flags in the workspace error
 * word; read them with gtf_read_errors().
 *
 * Which reference interface each entry point replaces (file:line in the
 * reference repository):
 *   gtf_extrapolate  -> src/extrapolate/extrapolate_merged_states.py:552-566
 *                       (message_passing :406-451 + extrapolate_validate :26-402,
 *                        compute_prior_probabilities + reweight x2, node degree)
 *   gtf_update       -> src/update/remove_state_metadata.py:29-53
 *   gtf_cluster      -> src/clustering/clustering.py:181-373 (cluster body)
 *   gtf_pass         -> the three above back to back, one fused node kernel
 *                       (run_gnn_trackml_mod.sh:101,138,112 stage order)
 *   gtf_tag_sweep    -> tag_propagation/tag_propagation.py:137-164 (one sweep)
 *   gtf_tag_prepare  -> tag_propagation/tag_propagation.py:97-110
 *   gtf_tag_propagate -> tag_propagation/tag_propagation.py:97-164 (the whole stage)
 *   gtf_tag_sweep_shard -> one sweep (:137-164) on an edge-sharded event
 *   gtf_comm_*, gtf_halo_exchange, gtf_halo_alltoall, gtf_allreduce_max_i64, gtf_allgather_bytes,
 *   gtf_tag_propagate_shard -> no reference counterpart: the collectives of one event
 *                       sharded over the GPUs of a node, in place of the
 *                       serial subgraph loop src/extrapolate/extrapolate_merged_states.py:406-451
 *   gtf_updated_state_distances -> calculate_distance_between_updated_states/
 *                       calculate_distance_between_updated_track_states.py:27-104,134-195
 *   gtf_score_reset, gtf_score_candidates, gtf_score_finish
 *                    -> src/extract/reconstruction_efficiency.py:118-183 (the candidates'
 *                       majority particles, the three tests, the match order and its counts)
 *   gtf_truth_concat, gtf_score_reset_ev, gtf_score_candidates_ev, gtf_score_finish_ev
 *                    -> the same lines for the K events of a fused graph in one call
 *   gtf_truth_build  -> src/extract/reconstruction_efficiency.py:41-91 (the reference tracks) and
 *                       utilities/helper.py:466-479 (hit_dissociation): the scorer's static tables
 *   gtf_csv_parse    -> the pd.read_csv / np.loadtxt calls in front of both
 *                       (utilities/helper.py:524-543, reconstruction_efficiency.py:41-47)
 *   gtf_event_window, gtf_event_radius_patch
 *                    -> utilities/helper.py:526-531 (the volume window) and :12-13 (r)
 *   gtf_graph_concat, gtf_concat_columns, gtf_candidate_order_device_ev, gtf_event_split
 *                    -> no reference counterpart: a batch of events as one graph, in place of
 *                       running run_gnn_trackml_mod.sh once per event
 *   gtf_kl_prepare, gtf_kl_coords, gtf_kl_pair_rows
 *                    -> learn_KL_parabolic_model/src/generate_training_data/
 *                       extract_metadata_trackml_parabolic_model.py:15-99 (the in-edges, their
 *                       pairs and the (node, i, j, emp_var) columns of a row), as
 *                       gtf/parabolic.py ParabolicKL restates them
 */
#ifndef GTF_H
#define GTF_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gtf_stream_t; /* a hipStream_t */

/* Version of the struct layouts below. gtf_graph carries it with its own size, and every
 * entry point taking a gtf_graph refuses a caller built against another layout
 * (status -3, gtf_last_error() names both). Bumped on every layout change. */
#define GTF_ABI_VERSION 8u

/* ---- graph structure (read-only on the path) ------------------------------ */
typedef struct gtf_graph {
    uint32_t struct_size;     /* sizeof(gtf_graph) as the caller compiled it */
    uint32_t abi_version;     /* GTF_ABI_VERSION */
    int32_t n_nodes;
    int32_t n_slots;          /* slots = (receiver, sender) pairs, receiver-major */
    int32_t n_edges;          /* directed edges = slots with is_edge == 1 */
    int32_t n_big;            /* schedule entries after the lane-group buckets (> 64 slots) */
    const int32_t* slot_ptr;  /* [N+1] slot segment of each receiver */
    const int32_t* slot_src;  /* [S]   sender node index, -1 = orphan state key */
    const int32_t* slot_dst;  /* [S]   receiver node index */
    const int32_t* out_ptr;   /* [N+1] out-edge segment of each sender */
    const int32_t* out_slot;  /* [E]   slot of each out-edge, successor order */
    const int32_t* slot_outpos; /* [S] position of the slot's edge in its sender's out-list (-1 = none) */
    const uint8_t* is_edge;   /* [S]   edge sender->receiver exists */
    const uint8_t* rev_edge;  /* [S]   edge receiver->sender exists */
    const uint8_t* solo;      /* [N]   node is alone in its subgraph */
    const double*  gnn;       /* [N*4] GNN_Measurement x,y,z,r */
    const double*  xyzr;      /* [N*4] node attribute 'xyzr' */
    const double*  layer;     /* [N]   in_volume_layer_id */
    /* optional node schedule for the node-local stages (NULL = one thread per node):
     * node indices bucketed by slot count -- n_g4 nodes with <= 4 slots (n_g4 is the LAST
     * field of this struct, added after the others), then n_g8 nodes with <= 8 slots,
     * n_g16 with 9..16, n_g32 with 17..32, n_g64 with 33..64 (a group of that many lanes
     * per node), then n_big nodes with more slots (one thread per node). Built once per
     * graph (gtf_graph_prepare, or gtf/device.py on the host); a shard's graph view holds the
     * schedule of its own receivers. */
    const int32_t* sched;     /* [N] */
    int32_t n_g8;
    int32_t n_g16;
    int32_t n_g32;
    int32_t n_g64;
    const int32_t* out_dst;   /* [E] receiver of each out-edge = slot_dst[out_slot] (saves the sender
                                 scan a dependent gather), or NULL */
    const double* slot_layer; /* [S] layer of each slot's sender (NaN for orphans) = layer[slot_src]:
                                 a coalesced read in the node kernels instead of a gather, or NULL */
    int32_t n_g4;             /* schedule entries before the n_g8 bucket: nodes with <= 4 slots
                                 (4 lanes per node; 0 = none, the n_g8 bucket then starts at 0) */
    const int32_t* sched_seg; /* [2*len(sched)] slot segment (slot_ptr[v], slot_ptr[v+1]) of each
                                 schedule entry v, read beside it: the node kernels then reach the
                                 slots without a dependent slot_ptr gather; or NULL */
    /* optional sender schedule for the var_ms scan (NULL = 8 lanes for every node): one
     * (sender, out_ptr[sender], out_ptr[sender+1], 0) int32 quadruple per sender with an
     * out-edge -- n_o4 senders with 1..4 out-edges (4 lanes each), then n_o8 with 5..8
     * (8 lanes), then n_o16 with more (16 lanes). Not used by gtf_pass_shard. */
    const int32_t* out_sched;  /* [4*(n_o4+n_o8+n_o16)] */
    int32_t n_o4;
    int32_t n_o8;
    int32_t n_o16;
    int32_t n_g2;             /* the first n_g2 entries of the n_g4 bucket have <= 2 slots and run on
                                 2 lanes per node in gtf_pass / the node ops (0 = all on 4 lanes) */
    /* optional packed schedule for gtf_pass's node kernel (replaces the lane-group buckets
     * there; the > 64-slot nodes still come from sched): wavefront w takes the entries
     * [pack_wave[w], pack_wave[w+1]) of pack_ent, each (v, slot_ptr[v], slot_ptr[v+1], first
     * lane) as int32 quadruples, one lane per slot (one for a slot-free node), <= 64 lanes. */
    const int32_t* pack_ent;  /* [4*n_entries] */
    const int32_t* pack_wave; /* [n_pack_waves+1] */
    int32_t n_pack_waves;
    /* optional per-lane view of out_sched's 4- and 8-lane buckets (v3): for lane l of entry e
     * of those buckets, (out_slot[o], receiver of o) with o = out_ptr[sender] + l, or (-1, 0)
     * past the sender's last out-edge, as int32 pairs -- the scan then reads each lane's edge
     * beside the schedule entry instead of after it (one dependent round of loads fewer).
     * [2 * (4 * n_o4 + 8 * n_o8)], or NULL. */
    const int32_t* out_lanes;
    /* optional padded tile layout of the node kernel (v3; gtf.graph.padded): the nodes of
     * each lane-group size G = 2, 4, 8, 16, 32, 64 own exactly G slots (their own, then inert
     * padding slots: orphan, no edge, rank -1 in both dicts), and each of pad_tiles tiles
     * holds pad_count[j] nodes of group j, groups in that order: node (t, j, i) is
     * t * pad_tile_nodes + sum(pad_count[:j]) + i, its slots start at t * pad_tile_slots +
     * sum(pad_count[:j] * G[:j]) + i * G[j]. Built with -DGTF_PAD_ARITH=1, gtf_pass's node
     * kernel then finds every node and slot by arithmetic (no schedule loads); the default
     * build reads the schedule (sched must list the nodes either way: the other entry points
     * and the > 64-slot nodes use it). pad_tiles = 0: none. */
    int32_t pad_tiles;
    int32_t pad_tile_nodes;
    int32_t pad_tile_slots;
    int32_t pad_count[6];
    int32_t pad_reserved_;
    /* optional (v4): global out-edge index of each slot's edge, out_ptr[slot_src] + slot_outpos
     * (-1 = no edge), or NULL. With it the sender scan stores the running merged_cov[1,1]
     * each extrapolation sees in out-edge order (contiguous per sender, coalesced stores)
     * and the extrapolation reads it through this index; NULL: stored by slot. [S] */
    const int32_t* slot_outidx;
    /* optional (v5): graph-static partitions of every receiver's slot segment, built once per
     * graph (gtf/device.py) so the node kernel does not rebuild them in every pass. For slot
     * k at position i of a segment of d <= 32 slots: bits 0..31 = the positions j of the
     * segment whose sender has slot k's sender layer (layer[slot_src], compute_prior_
     * probabilities' groups, helper.py:30-63; an orphan or NaN layer: {i}); bits 32..63 = the
     * positions whose sender's GNN_Measurement x equals slot k's sender's (the side norm's
     * distinct-x classes, helper.py:111-139, for entries whose stored x is the sender's live
     * GNN x -- see gtf_states.fresh); for a segment of 33..64 slots (v7) all 64 bits are the
     * same-layer positions and slot_xclass holds the same-x ones; 0 for larger segments. [S], or NULL
     * (the kernel then builds the classes itself). */
    const uint64_t* slot_class;
    /* optional (v5, with slot_class): bit 0 = the sender's GNN x < the receiver's GNN x (the
     * side of a live entry, helper.py:116-121). [S], or NULL. */
    const uint8_t* slot_sflags;
    /* optional (v7): the GNN_Measurement x, z, r of each slot's sender (gnn[4 slot_src + 0, 2, 3],
     * NaN for an orphan key), graph-static like slot_class. The coordinates of a live UTS entry
     * (gtf_states.fresh bit 1, extrapolate_merged_states.py:377) are its sender's GNN ones; the
     * node kernel's clustering stage (the tau geometry of the pairwise chi2, clustering.py:
     * 49-57) and the side norm read them here, contiguously per slot, instead of gathering the
     * sender's 32-byte gnn row per state. A caller that changes g->gnn refreshes it (or passes
     * NULL: the kernel then gathers gnn). [S*3], or NULL. */
    const double* slot_sxzr;
    /* optional (v7): one 32-bit word per slot of a receiver segment of d <= 8 slots, read by the
     * node kernel's lane groups of <= 8 lanes in place of four loads: bits 0..7 = slot_class bits
     * 0..7 (the same-layer positions), bits 8..15 = slot_class bits 32..39 (the same-x
     * positions), bit 16 = is_edge, bit 17 = rev_edge, bit 18 = slot_sflags bit 0; 0 for larger
     * segments. Graph-static, built with slot_class. [S], or NULL. */
    const uint32_t* slot_static;
    /* optional (v7, with slot_class): the same-x positions of the slots of 33..64-slot segments
     * (64 bits; slot_class then holds all 64 same-layer bits there), so the 64-lane groups read
     * their classes too instead of electing leaders per distinct value; 0 elsewhere. [S], or
     * NULL. */
    const uint64_t* slot_xclass;
    /* optional (v8): sub-buckets of the schedule for gtf_pass's fused node kernel. The first n_g6
     * entries of the n_g8 bucket have <= 6 slots and run on 6 lanes per node (10 nodes per
     * wavefront instead of 8); the first n_g12 entries of the n_g16 bucket have <= 12 slots and
     * run on 12 lanes (5 nodes per wavefront instead of 4). 0 = the whole bucket on 8 / 16
     * lanes. The other entry points take the buckets whole. */
    int32_t n_g6;
    int32_t n_g12;
} gtf_graph;

/* ---- per-node mutable state ------------------------------------------------ */
typedef struct gtf_nodes {
    uint8_t* has_merged;      /* [N] */
    double*  merged_state;    /* [N*3] a, b, c */
    double*  merged_cov;      /* [N*5] c00 c01 c10 c11 c22 (block diagonal) */
    double*  merged_prior;    /* [N] */
    uint8_t* has_tse;         /* [N] node has a 'track_state_estimates' dict */
    uint8_t* has_uts;         /* [N] node has an 'updated_track_states' dict */
    int32_t* degree;          /* [N] */
} gtf_nodes;

/* ---- one state dict (track_state_estimates or updated_track_states) -------- */
typedef struct gtf_states {
    int32_t* rank;            /* [S] dict position, -1 = key absent */
    double*  sv;              /* [S*3] edge_state_vector a, b, c */
    double*  tau;             /* [S]   joint_vector[2] */
    double*  cov;             /* [S*5] c00 c01 c10 c11 c22 */
    double*  xyzr;            /* [S*4] sender coordinates stored in the state */
    double*  lik;             /* [S]   likelihood (UTS only) */
    double*  mw;              /* [S]   mixture_weight */
    double*  prior;           /* [S]   prior */
    double*  lr;              /* [S]   lr_layer_norm (UTS only) */
    int8_t*  side;            /* [S]   0 left, 1 right (UTS only) */
    uint8_t* fresh;           /* [S]   UTS only: bit 0 = entry written by the last message passing;
                                 bit 1 = the entry's xyzr is its sender's live GNN coordinates
                                 gnn[slot_src] (extrapolate_merged_states.py:377 stores exactly
                                 those), so xyzr[k] itself is not written -- gtf_uts_materialize
                                 writes it (before a caller mutates g->gnn or reads uts->xyzr) */
} gtf_states;

/* ---- per-edge attributes (stored per slot) --------------------------------- */
typedef struct gtf_edges {
    uint8_t*      act;        /* [S] 'activated' */
    double*       edge_mw;    /* [S] edge 'mixture_weight' */
    const double* send_mw;    /* [S] sender's track_state_estimates[receiver]['mixture_weight'] */
} gtf_edges;

typedef struct gtf_params {
    double sigma0xy;          /* -e */
    double sigma0rz;          /* -z */
    double sigma0rz2;         /* -m */
    double endcap_boundary;   /* -b */
    double chi2_cut;          /* extrapolation gate -c (extrapolate_merged_states.py:298) */
    double reweight_threshold;/* 0.1 (helper.py:145) */
    double cluster_chi2;      /* clustering -c (clustering.py:228) */
    double cluster_kl;        /* clustering -k (clustering.py:261) */
} gtf_params;

/* Device-detected reference exceptions (bit flags in the error word). */
enum {
    GTF_ERR_SEND_MW_MISSING = 1,   /* KeyError extrapolate_merged_states.py:384 */
    GTF_ERR_STALE_KEY_NO_EDGE = 2, /* KeyError helper.py:131/138; the node's reweight goes on with lr_layer_norm = 1 for its active keys */
    GTF_ERR_ALL_ZERO_DIST = 4,     /* ValueError clustering.py:120 (np.min of empty); the node is left as it was: no merged state, no edge deactivated */
    GTF_ERR_TIE_EMPTIED = 8,       /* ValueError clustering.py:116 (tie removed every state) */
    GTF_ERR_EMPTY_DICT_MW = 16,    /* ZeroDivisionError helper.py:90; nothing is written for the node */
    GTF_ERR_NAN_KL = 32,           /* ValueError clustering.py:117 (list.index of NaN); the merged state formed so far is stored and the keys still in the list are deactivated */
    GTF_ERR_NO_STATE_DICT = 64,    /* KeyError remove_state_metadata.py:39 */
    GTF_ERR_SINGULAR_H = 128,      /* LinAlgError learn_KL_parabolic_model/.../utils.py:277 (x_B = 0 or x_B = x_0) and helper.py:384 (those and x_0 = 0; gtf_track_state_estimates_ws) */
    GTF_ERR_PAIR_COUNT = 256,      /* pair_ptr disagrees with the state dicts (caller error, a15) */
    GTF_ERR_NEIGHBOUR_MISSING = 512, /* KeyError calculate_distance_between_updated_track_states.py:182-183 */
    GTF_ERR_TOO_MANY_STATES = 1024 /* a15: a node with more than 2048 updated states (not processed) */
};

/* Workspace: caller allocates gtf_workspace_bytes() bytes of device memory and initialises
 * it once with gtf_workspace_init (or allocates it zeroed). Its first 8448 bytes are a
 * header: the error word at offset 0, the gtf_diag record at GTF_DIAG_OFFSET, and from byte
 * 256 the fused node kernel's work-queue counters (the kernel leaves them zero at the end of
 * every launch; only gtf_workspace_init or a zeroed allocation sets them up). One pass at a
 * time per workspace. */
size_t gtf_workspace_bytes(int32_t n_nodes, int32_t n_slots);

/* Zero the whole header (stream-ordered): no error flags, no diagnostics registered.
 * Required once on a workspace that was not allocated zeroed (hipMalloc): the kernels write
 * through every non-NULL gtf_diag pointer they find there. */
int gtf_workspace_init(void* workspace, gtf_stream_t stream);

/* Zero the error word only (stream-ordered); the registered diagnostics stay. */
int gtf_clear_errors(void* workspace, gtf_stream_t stream);

/* ---- Optional diagnostics outputs (SURVEY §5 "Metrics / logging"), off by default ----
 * The reference prints per-edge chi2 values to CSV files (extrapolate_merged_states.py
 * :143-172, the xy-plane chi2 of :134-140 is the one its gate uses) and raises exceptions
 * that abort a whole stage (the GTF_ERR_* places). Registered in the workspace by
 * gtf_set_diagnostics (NULL = all off), the pass kernels of that workspace then write:
 *   node_err[v]  |= the GTF_ERR_* bits of every reference exception node v raised
 *                  (gtf_pass / gtf_extrapolate / gtf_update / gtf_cluster / gtf_node_ops);
 *                  caller-zeroed uint32 [N]: which node (so which subgraph) would raise;
 *   edge_chi2[k]  = chi2 of the extrapolation of slot k's edge (every active out-edge of a
 *                  merged sender, accepted or not; untouched elsewhere), double [S];
 *   slot_cluster  = which states each clustered node merged and which it left (below).
 * The truth-based confusion counts of the reference's printouts (helper.py:186-225,
 * extrapolate_merged_states.py:496-518, clustering.py:342-369) follow on the host from
 * the masks (gtf/diagnostics.py). Nothing here is on the timed path: with no diagnostics
 * registered a kernel reads one uniform pointer. */
#define GTF_DIAG_OFFSET 64
typedef struct gtf_diag {
    uint32_t* node_err;       /* [N] device, or NULL */
    double*   edge_chi2;      /* [S] device, or NULL */
    uint8_t*  slot_cluster;   /* [S] device, or NULL: for every node that clustered (gtf_cluster,
                                 gtf_pass), 1 on the slots of the states merged into its merged
                                 state (clustering.py's edges_to_remain_active), 2 on the states
                                 left over, whose in-edges it deactivates (edges_to_deactivate);
                                 untouched elsewhere (caller-zeroed) */
    void*     reserved_[5];   /* zero */
} gtf_diag;
int gtf_set_diagnostics(void* workspace, const gtf_diag* d, gtf_stream_t stream);
/* Copy the error word to the host (synchronises the stream). */
int gtf_read_errors(void* workspace, uint32_t* flags, gtf_stream_t stream);

int gtf_extrapolate(const gtf_graph* g, gtf_nodes* n, gtf_states* uts, gtf_edges* e,
                    const gtf_params* p, void* workspace, gtf_stream_t stream);
/* message passing alone (extrapolate_merged_states.py:406-451): extrapolation of every
 * merged state along active out-edges, gate, Kalman update, UTS dict insertion
 * (GTF_OP_FRESH then GTF_OP_RANKS in the node kernel). */
int gtf_message_passing(const gtf_graph* g, gtf_nodes* n, gtf_states* uts, gtf_edges* e,
                        const gtf_params* p, void* workspace, gtf_stream_t stream);

/* Node-local helper operations, run in the given order for every node in one launch. */
enum {
    GTF_OP_RANKS = 1,        /* append keys created by message passing to the UTS dict */
    GTF_OP_PRIORS_TSE = 2,   /* helper.compute_prior_probabilities(.., 'track_state_estimates') :30-63 */
    GTF_OP_PRIORS_UTS = 3,   /* helper.compute_prior_probabilities(.., 'updated_track_states') */
    GTF_OP_REWEIGHT_UTS = 4, /* helper.reweight(.., 'updated_track_states') :143-225 */
    GTF_OP_DEGREE = 5,       /* node 'degree' = helper.query_node_degree_in_edges :67-73 */
    GTF_OP_PRUNE = 6,        /* remove_state_metadata.py:31-48 */
    GTF_OP_MW_TSE = 7,       /* helper.compute_mixture_weights(.., 'track_state_estimates') :76-96 */
    GTF_OP_MW_UTS = 8,
    GTF_OP_CLUSTER_TSE = 9,  /* clustering.py:197-321 on track_state_estimates */
    GTF_OP_CLUSTER_UTS = 10,
    GTF_OP_FRESH = 11        /* the entries message passing (re)wrote (uts.fresh): mixture_weight =
                                the sender's TSE weight (extrapolate_merged_states.py:384), prior / lr /
                                side absent; gtf_message_passing / gtf_extrapolate / gtf_pass run it */
};
/* ops: host array of n_ops (<= 24) GTF_OP_* codes; thresholds used by the cluster ops. */
int gtf_node_ops(const gtf_graph* g, gtf_nodes* n, gtf_states* tse, gtf_states* uts, gtf_edges* e,
                 const gtf_params* p, const int8_t* ops, int32_t n_ops, double chi2_threshold,
                 double kl_threshold, void* workspace, gtf_stream_t stream);
int gtf_update(const gtf_graph* g, gtf_nodes* n, gtf_states* tse, gtf_states* uts, gtf_edges* e,
               const gtf_params* p, void* workspace, gtf_stream_t stream);
/* key: 0 = cluster track_state_estimates, 1 = updated_track_states. Where a
 * distance tie empties the state list the reference raises ValueError; here the
 * node keeps the merged state formed so far and GTF_ERR_TIE_EMPTIED is set. */
int gtf_cluster(const gtf_graph* g, gtf_nodes* n, gtf_states* states, gtf_edges* e, int32_t key,
                double chi2_threshold, double kl_threshold, const gtf_params* p, void* workspace,
                gtf_stream_t stream);
/* Write gnn[slot_src] into uts->xyzr of every entry whose xyzr is live (uts->fresh bit 1) and
 * clear that bit: the stored snapshot extrapolate_merged_states.py:377 makes. Call it before
 * mutating g->gnn (extraction's close-proximity merge, extract_track_candidates.py:111-118)
 * and before reading uts->xyzr back. */
int gtf_uts_materialize(const gtf_graph* g, gtf_states* uts, gtf_stream_t stream);

/* extrapolate -> update -> cluster(updated_track_states, p->cluster_chi2, p->cluster_kl) */
int gtf_pass(const gtf_graph* g, gtf_nodes* n, gtf_states* tse, gtf_states* uts, gtf_edges* e,
             const gtf_params* p, void* workspace, gtf_stream_t stream);
/* gtf_pass with hipEvent_t events[5] recorded on the stream before the sender scan,
 * after it, after the edge extrapolation kernel, after the fused node kernel (priors,
 * reweights, update and KL clustering in one launch) and at the end of the pass
 * (per-kernel timing for the roofline report; events may be NULL). */
int gtf_pass_ev(const gtf_graph* g, gtf_nodes* n, gtf_states* tse, gtf_states* uts, gtf_edges* e,
                const gtf_params* p, void* workspace, gtf_stream_t stream, void* const* events);

/* ---- One event sharded across GPUs --------------------------------
 * Rank r owns a contiguous receiver range [node_lo, node_hi) and so the contiguous slot
 * range [slot_lo, slot_hi) (slots are receiver-major); every rank holds the whole graph.
 * gtf_pass_shard runs the pass for the owned receivers: the sender scan over `senders`
 * (every sender with an out-edge into an owned receiver, plus the owned senders whose
 * merged_cov write-back the rank publishes), extrapolation of the owned slots, and the
 * node kernels over the owned receivers (pass `g` with sched, n_g8..n_g64 and n_big describing the
 * owned receivers only; with g->out_sched set, the scan runs on that out-degree-bucketed
 * schedule of the shard's senders). Between passes the ranks exchange what the next pass
 * reads: the halo (gtf_halo_pack -> all-to-all -> gtf_halo_unpack, below), or every owned
 * state (gtf_shard_pack -> an all-gather of equal-size chunks -> gtf_shard_unpack: full
 * replicas, used before reading results back). */
typedef struct gtf_shard {
    const int32_t* senders;   /* [n_senders] device */
    int32_t n_senders;
    int32_t node_lo, node_hi;
    int32_t slot_lo, slot_hi;
    /* ABI v6: the pass in phases, so the halo exchange can overlap the part that does not
     * read it (gtf.shard.ShardedDeviceGraph.step). phases = 0 (or 3): the whole pass; 1: the
     * sender scan over `senders` and the extrapolation only; 2: the node kernels only; 5 (1 |
     * 4): phase 1 fused sender-major -- every out-edge of `senders` into [slot_lo, slot_hi)
     * extrapolated by its scan lane right after the scan (one launch; needs g->out_sched;
     * slot_list unused).
     * slot_list (device, ascending, [n_slot_list]) or NULL: phase 1 extrapolates exactly these
     * owned slots instead of [slot_lo, slot_hi). A rank's pass as two phase-1 calls (the
     * senders whose state and out-edge activations are all its own, with the slots they
     * send to; then the rest, after the exchange) and one phase-2 call equals the one-call
     * pass bit for bit: every sender is scanned once, in its own successor order, and every
     * owned slot extrapolated once. */
    int32_t phases;
    const int32_t* slot_list;
    int32_t n_slot_list;
    int32_t pad_;
} gtf_shard;

int gtf_pass_shard(const gtf_graph* g, gtf_nodes* n, gtf_states* tse, gtf_states* uts, gtf_edges* e,
                   const gtf_params* p, const gtf_shard* shard, void* workspace, gtf_stream_t stream,
                   void* const* events);
/* bytes of one rank's chunk holding up to cap_nodes node states and cap_slots activations */
size_t gtf_shard_chunk_bytes(int32_t cap_nodes, int32_t cap_slots);
/* write the owned nodes' has_merged / merged_state / merged_cov / merged_prior and the
 * owned slots' activation into chunk (device) */
int gtf_shard_pack(const gtf_nodes* n, const gtf_edges* e, const gtf_shard* shard, int32_t cap_nodes,
                   int32_t cap_slots, void* chunk, gtf_stream_t stream);
/* scatter the chunks of all ranks except `self` (gathered: nranks chunks back to back);
 * ranges: device int32 [4 * nranks] = node_lo, node_hi, slot_lo, slot_hi per rank */
int gtf_shard_unpack(gtf_nodes* n, gtf_edges* e, const void* gathered, int32_t nranks, int32_t self,
                     const int32_t* ranges, int32_t cap_nodes, int32_t cap_slots, gtf_stream_t stream);

/* Halo exchange (the per-pass exchange of gtf/shard.py): only what the other ranks' next
 * pass reads -- the merged state of their halo senders owned here, and the activation
 * of the out-edges of their senders whose receivers are owned here -- instead of every
 * owned state. The lists are built once per plan (host); per pass a rank packs one
 * buffer of per-destination segments, exchanges it with one all-to-all (RCCL over
 * xGMI), and scatters what it received. A node record is GTF_HALO_NODE_BYTES: has_merged
 * as a 64-bit integer, merged_state[3], merged_cov[5], merged_prior (raw fp64 bits);
 * an activation is one byte. Offsets of node records must be multiples of 8. */
#define GTF_HALO_NODE_BYTES 80
typedef struct gtf_halo {
    const int32_t* node_idx;  /* [n_nodes] device: node of each record */
    const int64_t* node_off;  /* [n_nodes] device: byte offset of each record in the buffer */
    int32_t n_nodes;
    int32_t pad_;
    const int32_t* slot_idx;  /* [n_slots] device: slot of each activation byte */
    const int64_t* slot_off;  /* [n_slots] device: byte offset of each activation byte */
    int32_t n_slots;
    int32_t pad2_;
} gtf_halo;
/* gather the listed node states and activations into buf (device) */
int gtf_halo_pack(const gtf_nodes* n, const gtf_edges* e, const gtf_halo* h, void* buf, gtf_stream_t stream);
/* scatter buf (device) into the listed node states and activations */
int gtf_halo_unpack(gtf_nodes* n, gtf_edges* e, const gtf_halo* h, const void* buf, gtf_stream_t stream);

/* Tag propagation. radius: [N] node radius (attr 'zr'[1]); keep: [E] output mask of
 * kept inward neighbours per out-edge (u8, indexed by out-edge position);
 * processed: [N] u8 output; n_processed: device int32 output. With g->out_sched set the
 * prepare runs on its lane groups, so that schedule must list every node with an out-edge
 * (not a shard's restricted one: pass the graph without out_sched then). */
int gtf_tag_prepare(const gtf_graph* g, const double* radius, uint8_t* keep, uint8_t* processed,
                    int32_t* n_processed, gtf_stream_t stream);
/* one Jacobi sweep: tags_out[u] = max(tags_in[u], tags_in[kept neighbours]); *flips = the
 * number of changed tags (zeroed first). With g->out_sched (and out_lanes) the sweep runs
 * on the sender schedule's lane groups, otherwise one thread per node. */
int gtf_tag_sweep(const gtf_graph* g, const uint8_t* keep, const uint8_t* processed,
                  const int64_t* tags_in, int64_t* tags_out, int32_t* flips, gtf_stream_t stream);
/* The whole tag-propagation stage in one call (tag_propagation.py:97-164: prepare, then
 * sweeps while flips / processed > flip_threshold -- the reference's 0.1 -- and fewer than
 * max_sweeps; the first sweep always runs). tags: device int64 [n_nodes], the initial tags
 * in, the final tags out; flips_out: host int32 [max_sweeps] (or NULL), the flip count of
 * every sweep; *sweeps_out: the number of sweeps. workspace: device, at least
 * gtf_tag_workspace_bytes(n_nodes, n_edges) bytes. The prepare launch builds a compact list
 * of every node's kept out-neighbours in the workspace, and the sweeps read those lists with
 * the tags carried as int32 while every tag fits (int64 from the first value that does not;
 * environment GTF_TAG_CSR=0: the keep-mask sweeps of gtf_tag_sweep). The sweeps go out in
 * batches of 4, 8, 16, ... 64 launches with the stop rule evaluated on the device; the host
 * waits once per batch, for a small report (the stop-rule words and the batch's flip totals)
 * the device writes into mapped page-locked memory the host polls (environment
 * GTF_TAG_POLL=0: a device-to-host copy and a stream synchronisation instead). */
size_t gtf_tag_workspace_bytes(int32_t n_nodes, int32_t n_edges);
int gtf_tag_propagate(const gtf_graph* g, const double* radius, int64_t* tags, double flip_threshold,
                      int32_t max_sweeps, int32_t* flips_out, int32_t* sweeps_out, void* workspace,
                      size_t workspace_bytes, gtf_stream_t stream);
/* One rank's sweep of tag propagation on an edge-sharded event (the sweep of
 * tag_propagation.py:137-164 over the rank's owned nodes [shard->node_lo, shard->node_hi)
 * of the replicated graph `g`). tags_in / tags_out: device int64 [n_nodes + nranks].
 * Writes the owned nodes' next tags, INT64_MIN for every other node, this rank's flip count
 * to tags_out[n_nodes + rank] and 0 to the other ranks' count words, so ONE all-reduce(MAX)
 * of the n_nodes + nranks words gives every rank the whole next tag array and every
 * rank's flip count (their sum is the sweep's flips). gtf_tag_prepare runs unsharded on
 * the replica (its n_processed is the whole event's). */
int gtf_tag_sweep_shard(const gtf_graph* g, const uint8_t* keep, const uint8_t* processed,
                        const int64_t* tags_in, int64_t* tags_out, const gtf_shard* shard,
                        int32_t rank, int32_t nranks, gtf_stream_t stream);

/* ---- Native collectives for the sharded event (SURVEY §8b gtf_comm_init, §8e) ----------
 * RCCL over xGMI inside libgtf, one communicator per rank (one process per GPU; create it
 * with the rank's device current), every call stream-ordered on the caller's stream. RCCL is
 * loaded on first use (GTF_RCCL = its path, else an RCCL already loaded in the process, else
 * librccl.so.1). Rank 0 calls gtf_comm_unique_id and hands the GTF_COMM_ID_BYTES to the other
 * ranks (file, socket, MPI, ...); each rank then calls gtf_comm_init. Status -4: an RCCL
 * error (gtf_last_error names it). These replace the role of the reference's serial subgraph
 * loop (src/extrapolate/extrapolate_merged_states.py:406-451) for one event spread over the
 * GPUs of a node. */
#define GTF_COMM_ID_BYTES 128
typedef struct gtf_comm gtf_comm;
int gtf_comm_unique_id(void* id);
int gtf_comm_init(gtf_comm** comm, int32_t rank, int32_t nranks, const void* rccl_uid);
int gtf_comm_destroy(gtf_comm* comm);
int gtf_comm_rank(const gtf_comm* comm);
int gtf_comm_size(const gtf_comm* comm);
/* The per-pass halo exchange: gtf_halo_pack into send_buf, one all-to-all of the
 * per-destination segments (send_bytes[p] / recv_bytes[p]: host int64 [nranks], segments back
 * to back in rank order, a rank's own segment empty), gtf_halo_unpack from recv_buf. */
int gtf_halo_exchange(gtf_comm* comm, gtf_nodes* n, gtf_edges* e, const gtf_halo* send, const gtf_halo* recv,
                      void* send_buf, void* recv_buf, const int64_t* send_bytes, const int64_t* recv_bytes,
                      gtf_stream_t stream);
/* the all-to-all of gtf_halo_exchange alone (no pack / unpack), for a caller that runs it on
 * a stream of its own beside the pass's phase 1 (gtf_shard.phases) */
int gtf_halo_alltoall(gtf_comm* comm, const void* send_buf, void* recv_buf, const int64_t* send_bytes,
                      const int64_t* recv_bytes, gtf_stream_t stream);
/* in-place all-reduce(MAX) of int64 words (the sharded tag sweep's exchange) */
int gtf_allreduce_max_i64(gtf_comm* comm, int64_t* words, int64_t count, gtf_stream_t stream);
/* all-gather of one equal-size chunk per rank into gathered (nranks chunks, rank order):
 * gtf_shard_pack -> this -> gtf_shard_unpack completes every replica */
int gtf_allgather_bytes(gtf_comm* comm, const void* chunk, void* gathered, int64_t bytes, gtf_stream_t stream);
/* The whole tag-propagation stage on an edge-sharded event (tag_propagation.py:97-164): prepare
 * on the replica, per sweep gtf_tag_sweep_shard over the owned nodes + one all-reduce(MAX),
 * stop when flips / processed <= flip_threshold (one synchronisation per sweep). tags: device
 * int64 [n_nodes] in / out (every rank ends with the whole array). */
size_t gtf_tag_shard_workspace_bytes(int32_t n_nodes, int32_t n_edges, int32_t nranks);
int gtf_tag_propagate_shard(gtf_comm* comm, const gtf_graph* g, const gtf_shard* shard, const double* radius,
                            int64_t* tags, double flip_threshold, int32_t max_sweeps, int32_t* flips_out,
                            int32_t* sweeps_out, void* workspace, size_t workspace_bytes, gtf_stream_t stream);

/* ---- Distances between updated track states --------------------
 * calculate_distance_between_updated_states/calculate_distance_between_updated_track_states.py:
 * mahalanobis_distance (:27-104) over the pair loop of :134-195. For every node with an
 * updated_track_states dict (n->has_uts, :143) and more than one active in-edge (:139-140),
 * every pair i > j of its dict entries in dict order (:174-176): the [a, b] Mahalanobis term
 * plus the delta-tau term with the hard-coded sigma_z = 0.5 / sigma_r = 0.1, swapped where
 * |x| >= 600 (:62-74); <tau>, <theta>, delta theta (:89-99); and the truth flag (:190-193).
 * Coordinates: g->xyzr of the node and of each neighbour (:162-163, :182-183).
 * Pairs of node v are written at [pair_ptr[v] + t], t = i (i - 1) / 2 + j (the reference's
 * loop order). gtf_updated_state_pair_counts writes each node's pair count (0 or d(d-1)/2)
 * for the caller's exclusive scan into pair_ptr [N+1]; a node whose pair_ptr range has
 * another size is skipped with GTF_ERR_PAIR_COUNT. Uses g->sched when present; with
 * g->sched == NULL every node runs on the one-wavefront path, to the same bits.
 * A pair whose C_i + C_j is exactly singular (the reference's np.linalg.inv raises
 * LinAlgError, :37) raises nothing here: its chi2 is left non-finite (NaN or +-inf), its
 * other columns are what they are for any pair, and no other pair is affected. Where r of
 * a neighbour equals the node's r the columns are non-finite in the reference's kind.
 * A node that raises an error bit (a pair_ptr range of another size; a present key with
 * slot_src < 0, the KeyError of :182-183; more than 2048 keys) has none of its pairs
 * written; every other node of the call is. */
typedef struct gtf_pair_out {
    double* chi2;         /* [P] */
    double* avg_tau;      /* [P] or NULL */
    double* avg_theta;    /* [P] or NULL */
    double* delta_theta;  /* [P] or NULL */
    int8_t* truth;        /* [P] or NULL (needs node truth) */
    uint32_t* err;        /* device error word (GTF_ERR_PAIR_COUNT / _NEIGHBOUR_MISSING / _TOO_MANY_STATES) or NULL */
} gtf_pair_out;

int gtf_updated_state_pair_counts(const gtf_graph* g, const gtf_nodes* n, const gtf_states* uts, const gtf_edges* e,
                                  int64_t* counts, gtf_stream_t stream);
/* truth: [N] truth_particle per node (device), or NULL */
int gtf_updated_state_distances(const gtf_graph* g, const gtf_nodes* n, const gtf_states* uts, const gtf_edges* e,
                                const int64_t* truth, const int64_t* pair_ptr, const gtf_pair_out* out,
                                gtf_stream_t stream);

/* ---- Initial track-state estimates -----------------------------
 * helper.compute_track_state_estimates (helper.py:238-452): for every key of every
 * node's track_state_estimates dict (slots with tse->rank >= 0; the dict order is an
 * input, the reference's reversed(set(nx.all_neighbors)) order) writes tse->sv
 * (edge_state_vector), tse->cov (the aliased edge/joint covariance, :417-425),
 * tse->tau (joint_vector[2]) and tse->xyzr (neighbour coordinates), plus the optional
 * per-slot / per-node extras below. Needs g->sched (the slot-count node schedule).
 * The reference reads its set-ordered tau / del_tau / theta lists with dict positions
 * (:384, :419-431); that pairing is reproduced. */
typedef struct gtf_tse_extra {
    double* theta;        /* [S*3] theta, theta2, variance_theta, or NULL */
    double* var_ms;       /* [S]   var_ms_node, or NULL */
    double* xy_mean_var;  /* [N*2] xy_edge_gradient_mean_var, or NULL */
    double* zr_mean_var;  /* [N*2] zr_edge_gradient_mean_var, or NULL */
    double* angle;        /* [N]   angle_of_rotation, or NULL */
    double* translation;  /* [N*2] translation, or NULL */
} gtf_tse_extra;

int gtf_track_state_estimates(const gtf_graph* g, gtf_states* tse, const gtf_tse_extra* extra,
                              const gtf_params* p, gtf_stream_t stream);
/* The same with the reference's exception reported. np.linalg.inv(H) raises LinAlgError
 * (helper.py:384) for a key whose parabola matrix is singular: x_B == 0 (the neighbour has the
 * node's own x, y), x_B == x_0 (the neighbour lies at the origin) or x_0 == 0 (the node lies
 * at the origin), compared on the fp64 values. With workspace != NULL (an initialised
 * gtf_workspace_bytes() block) the key's node then raises GTF_ERR_SINGULAR_H as the pass
 * kernels raise: into the workspace's error word and, where gtf_diag.node_err is registered,
 * into the node's entry. What the singular key's own outputs hold (sv, cov, tau, xyzr, theta,
 * var_ms) is unspecified; every other key of the node, the node's per-node outputs and every
 * other node are what they are without the singular key raising.
 * One singular key is NOT reported: a key that is the node itself (slot_src == the node), which
 * a self loop among the edge rows leaves in the dict (the builders keep such rows, as networkx
 * does). The reference raises there as well (x_B == 0); the pipelines have always converted
 * such events and gone on, the self key's own states being non-finite and every other state
 * exact, and that stays so. A caller that wants the reference's stop tests slot_src itself.
 * workspace == NULL is
 * gtf_track_state_estimates: nothing is reported. No output array changes with the workspace,
 * and a call in which no key is singular writes nothing to it.
 * Non-finite results have the reference's kind: where r or x of node and neighbour coincide
 * the reference's dense J S2 J^T multiplies infinities by zeros, so del_tau^2 and
 * variance_theta are NaN there, not +inf.
 * The node sums (np.mean / np.var of the gradients) are numpy's pairwise sums at every key
 * count, its recursion beyond 128 terms included. */
int gtf_track_state_estimates_ws(const gtf_graph* g, gtf_states* tse, const gtf_tse_extra* extra,
                                 const gtf_params* p, void* workspace, gtf_stream_t stream);

/* ---- Track-candidate extraction ---------------------------
 * src/extract/extract_track_candidates.py main (:349-467) on the pass's output: CCA
 * over the activated edges of each subgraph (a subgraph with no deactivated edge stays
 * one candidate), then per candidate the fragment check, close-proximity merging (the
 * reference mutates the merged node's GNN_Measurement in place, :111-114: io->gnn is
 * updated the same way), the one-hit-per-layer check, rotate_track and the xy / rz
 * Kalman fits with their chi-square p-values; a candidate is extracted when both
 * p-values reach p_accept. Candidates are identified by their first node (min index). */
typedef struct gtf_extract_params {
    double p_accept;          /* -p */
    int32_t fragment;         /* -n minimum hits (>= 3) */
    int32_t pad_;
    double separation_3d;     /* -s (rotate_track) */
    double merge_distance;    /* -t (close-proximity merging) */
    double sigma0xy, sigma0rz, endcap_boundary;   /* -e -z -b */
} gtf_extract_params;

typedef struct gtf_extract_io {
    const double* xyzr;       /* [N*4] node attribute xyzr */
    const double* vivl;       /* [N*2] volume_id, in_volume_layer_id */
    const int32_t* sub_id;    /* [N]   subgraph of each node (nodes grouped by subgraph) */
    const int32_t* sub_ptr;   /* [n_sub+1] first node of each subgraph */
    int32_t n_sub;
    int32_t pad_;
    const int32_t* order_key; /* [N] member order inside a candidate (distinct values), or NULL = node order */
    double* gnn;              /* [N*4] GNN_Measurement x,y,z,r: merged nodes get the midpoint */
    int32_t* label;           /* [N] out: candidate id of each node */
    int8_t* status;           /* [N] out per candidate id: 0 fragment, 1 bad layers, 2 rejected, 3 extracted */
    double* pval_xy;          /* [N] out per candidate id (NaN when not fitted) */
    double* pval_zr;
    uint8_t* extracted;       /* [N] out per node */
    int32_t* n_candidates;    /* device scalar out */
} gtf_extract_io;

size_t gtf_extract_workspace_bytes(int32_t n_nodes, int32_t n_sub);
/* synchronises the stream once per connected-components round (a few rounds); -1 with
 * "CCA did not converge" when none of 64 rounds passed without a change */
int gtf_extract_candidates(const gtf_graph* g, const gtf_edges* e, const gtf_extract_io* io,
                           const gtf_extract_params* p, void* workspace, gtf_stream_t stream);
/* Workspace contract: after a successful call the workspace holds the member list sorted by
 * (candidate id, order key) and the candidate pointers into it. gtf_extract_outputs (below)
 * reads them there, for the same n_nodes and n_sub; they are valid until the caller reuses
 * or frees the workspace. */

/* ---- The extraction's inputs and outputs without the host (resident loop) ---------------
 * gtf_subgraph_ptr_device: sub_ptr [n_sub + 1] (first node of each subgraph) from a device
 * sub_id [N] that numbers the subgraphs 0, 1, 2, ... with the nodes grouped (pack() order, a
 * gtf_graph_subset_apply result). Synchronises once; -2 when sub_id is not of that form or
 * does not end at n_sub - 1. n_nodes == 0: every pointer is 0 (no synchronisation). */
int gtf_subgraph_ptr_device(const int32_t* sub_id, int32_t n_nodes, int32_t n_sub, int32_t* sub_ptr,
                            gtf_stream_t stream);

/* gtf_candidate_order_device: gtf_candidate_order (below; extract_track_candidates.py:332-346)
 * from device arrays, the same order_key [N] array for array. Reads n_nodes, n_slots,
 * n_edges, slot_ptr, slot_src, slot_dst, out_ptr, out_slot and is_edge of *g, e->act, sub_id
 * [N] / sub_ptr [n_sub + 1] (as gtf_extract_io) and node_id [N] (int64, device).
 *   - a subgraph without an inactive edge: order_key[v] = v - sub_ptr[s] (:342-343);
 *   - else the components over the edges with act != 0 (the host function's rule; the
 *     extraction itself hooks act == 1), by the extraction's hook + compress rounds, their
 *     members by one radix sort of (component, node index);
 *   - a component of at least half its subgraph: the rank of the node index among its
 *     members (G.subgraph(c) iterates G when 2|c| >= |G|);
 *   - a smaller one ("set-ordered"): ONE THREAD walks the reference's BFS from the
 *     component's first node (successors in out_slot order, then predecessors in slot
 *     order), inserts node_id into a CPython 3.10 set, copies it into a second one
 *     (show_nodes(set(c))) and ranks the nodes in that set's iteration order. A very large
 *     component below half its subgraph is therefore slow but correct -- the limit of
 *     gtf_build_event_csr_device's component order; counts->max_set_ordered reports the
 *     largest one met.
 * node ids must be distinct and in [0, 2^61 - 1) (gtf_build_event_csr_device's rule), checked
 * on the device: -2. Null arguments (-2) and another ABI (-3) are decided on the host before
 * any launch. Synchronises `stream` once per hook round and once at the end, when *counts
 * is filled. n_nodes == 0: returns 0 with zero counts, nothing launched. */
typedef struct gtf_order_counts {
    int32_t n_components;      /* components over the act != 0 edges (whole graph) */
    int32_t n_set_ordered;     /* of them: ordered by the one-thread set walk */
    int32_t max_set_ordered;   /* nodes of the largest of those (0 when none) */
    int32_t pad_;
} gtf_order_counts;

/* positive for an empty graph, non-decreasing in every argument (negative counts as 0); the
 * set tables take <= 24 n_nodes words (3 tables of <= 8 max(k, 1) entries per component) */
size_t gtf_candidate_order_workspace_bytes(int32_t n_nodes, int32_t n_slots, int32_t n_sub);
int gtf_candidate_order_device(const gtf_graph* g, const gtf_edges* e, const int32_t* sub_id,
                               const int32_t* sub_ptr, int32_t n_sub, const int64_t* node_id,
                               int32_t* order_key, void* workspace, size_t workspace_bytes,
                               gtf_order_counts* counts, gtf_stream_t stream);
/* The same on a batch of events (gtf_graph_concat): `event` [N] (device) names the event of
 * every node, and node ids must be distinct within an event only -- the ids of different
 * events collide, and they cannot be shifted apart because the set order of a small component
 * hashes the id itself. The id -> node map is sorted by (event, id) instead of id (two stable
 * radix sorts) and a set-ordered component looks its ids up among its own event's. Any int32
 * values, in any node order. event == NULL: gtf_candidate_order_device, which is this call
 * with NULL. Same workspace size, same statuses and messages. */
int gtf_candidate_order_device_ev(const gtf_graph* g, const gtf_edges* e, const int32_t* sub_id,
                                  const int32_t* sub_ptr, int32_t n_sub, const int64_t* node_id,
                                  const int32_t* event, int32_t* order_key, void* workspace,
                                  size_t workspace_bytes, gtf_order_counts* counts, gtf_stream_t stream);

/* gtf_extract_outputs: the stage's outputs (extract_track_candidates.py:423-430 the remaining
 * and fragment subgraphs, :459-467 the node removal; gtf/extract.py outputs) from the results
 * of a gtf_extract_candidates call: label, status, extracted, pval_xy, pval_zr, sub_id,
 * sub_ptr, n_sub and n_candidates of *io, and the sorted member list and candidate pointers
 * that call left in `extract_workspace` (see the contract above). Device pointers,
 * caller-allocated at the upper bounds; all but left / keep may be NULL = not wanted. */
typedef struct gtf_extract_out {
    int32_t* left;           /* [n_sub]  nodes of each subgraph that were not extracted */
    uint8_t* keep;           /* [N]      1 = not extracted and left[sub] >= fragment: gtf_graph_subset_plan's mask */
    int32_t* cand_ptr;       /* [<= N+1] extracted candidates, in candidate-id order ... */
    int32_t* cand_members;   /* [<= N]   ... members in order-key order */
    double* pval_xy;         /* [<= N]   per extracted candidate, copied bit for bit */
    double* pval_zr;
    int32_t* rem_ptr;        /* [<= N+1] subgraphs with left >= fragment, in subgraph order ... */
    int32_t* rem_nodes;      /* [<= N]   ... their nodes that were not extracted, in node order */
    int32_t* frag_ptr;       /* [<= N+1] subgraphs with 0 < left < fragment */
    int32_t* frag_nodes;     /* [<= N] */
    const int64_t* node_id;  /* [N] or NULL; when set, the member arrays also as node ids: */
    int64_t* cand_ids;       /* [<= N] */
    int64_t* rem_ids;        /* [<= N] */
    int64_t* frag_ids;       /* [<= N] */
} gtf_extract_out;

typedef struct gtf_extract_out_counts {
    int32_t n_extracted, n_extracted_nodes;
    int32_t n_remaining, n_remaining_nodes;
    int32_t n_fragments, n_fragment_nodes;
} gtf_extract_out_counts;

/* positive for an empty graph, non-decreasing in both arguments */
size_t gtf_extract_outputs_workspace_bytes(int32_t n_nodes, int32_t n_sub);
/* Scans only (no atomics); synchronises `stream` once, when *counts is filled. -3 for another
 * ABI, -2 for a null argument, fragment < 1 or a small workspace, before any launch.
 * n_nodes == 0: returns 0 with zero counts, nothing launched, nothing written. */
int gtf_extract_outputs(const gtf_graph* g, const gtf_extract_io* io, int32_t fragment,
                        const void* extract_workspace, const gtf_extract_out* out, void* workspace,
                        size_t workspace_bytes, gtf_extract_out_counts* counts, gtf_stream_t stream);

/* ---- Candidate scoring: reconstruction efficiency and purities ---------------------
 * src/extract/reconstruction_efficiency.py:118-183 (gtf/metrics.py majority and
 * reconstruction_efficiency) on the device arrays gtf_extract_outputs leaves: cand_ptr /
 * cand_ids go straight into gtf_score_candidates, once per iteration, and gtf_score_finish
 * returns the matched particles in the script's match order. Everything is integer; the
 * caller forms the purities n_good / total and n_good / hits in fp64, so they are the
 * host's divisions bit for bit. gtf_score.hip.
 *
 * The three tests of :150-163 in integers: n_good >= 0.5 * hits, n_good / total >= 0.5 and
 * n_good / hits >= 0.5 are 2 n_good >= hits and 2 n_good >= total, because 0.5 and every
 * count here (< 2^31) are exact in fp64, 0.5 * hits is exact, and a correctly rounded
 * quotient n / t is monotone in the real quotient with 0.5 representable: n / t >= 0.5 in
 * fp64 exactly when n / t >= 1/2 in the rationals. (t == 0 gives NaN there and never passes:
 * an empty candidate never passes here.)
 *
 * gtf_truth: the event's static truth tables, DEVICE arrays built once per event: by
 * gtf_truth_build below from the parsed columns on the device, or by the caller on the host
 * and uploaded (gtf/metrics.py truth_tables: reconstruction_efficiency.py:41-91 the reference
 * tracks, helper.py:466-479 hit_dissociation; the definition of both). reference_tracks returns the same count array
 * for a particle's "reference hits" and its "region hits" (nhits[good] and nhits of one
 * np.unique), so ONE count per particle, part_hits, serves both thresholds. Particle ids
 * are arbitrary int64 (0 = noise occurs); both id arrays ascend as signed int64. */
typedef struct gtf_truth {
    uint32_t struct_size;       /* sizeof(gtf_truth) as the caller compiled it */
    uint32_t abi_version;       /* GTF_ABI_VERSION */
    int32_t n_nodes;            /* T: nodes with a hit_dissociation */
    int32_t n_entries;          /* P: particle entries of all of them */
    int32_t n_particles;        /* R: region particles */
    int32_t pad_;
    const int64_t* node_id;     /* [T]   ascending, distinct */
    const int32_t* node_ptr;    /* [T+1] CSR over node_part */
    const int64_t* node_part;   /* [P]   the particle of each hit of the node, in the node's hit order */
    const int64_t* part_id;     /* [R]   ascending, distinct */
    const int32_t* part_hits;   /* [R]   the particle's hits in the region (= its reference hits) */
    const uint8_t* part_ref;    /* [R]   1 = reference track */
} gtf_truth;

/* gtf_score_state: what the calls accumulate, DEVICE arrays owned by the caller. */
typedef struct gtf_score_state {
    int32_t n_particles;        /* R of the gtf_truth it is used with */
    int32_t pad_;
    uint64_t* best_key;         /* [R] (group << 32) | candidate index of the claim; all-ones = none */
    int32_t* best_good;         /* [R] n_good of the claiming candidate */
    int32_t* best_total;        /* [R] its number of particle entries */
    uint32_t* error;            /* [1] GTF_SCORE_ERR_* */
} gtf_score_state;

#define GTF_SCORE_ERR_MISSING   1u   /* a member id with no row in node_id */
#define GTF_SCORE_ERR_WORKSPACE 2u   /* cand_ptr[n_cand] members do not fit the workspace given */
#define GTF_SCORE_ERR_RANGE     4u   /* a candidate of 2^31 or more particle entries, or a decreasing cand_ptr */

/* Optional per-candidate results of gtf_score_candidates (gtf/metrics.py majority,
 * reconstruction_efficiency.py:132-134), DEVICE arrays [n_cand]; NULL = not wanted. */
typedef struct gtf_score_out {
    int64_t* pid;               /* the most frequent particle id, ties to the id seen first; 0 when empty */
    int32_t* n_good;            /* its count */
    int32_t* total;             /* the candidate's particle entries */
    uint8_t* passes;            /* 1 = reference track and both thresholds (before "first one wins") */
} gtf_score_out;

typedef struct gtf_score_counts {
    int32_t n_reconstructed;
    uint32_t error;             /* the state's error word */
} gtf_score_counts;

/* reconstruction_efficiency.py:118-121 (the empty tallies): every key all-ones, the error word
 * cleared. Two stream-ordered fills; does not synchronise. -2 for a null state or array. */
int gtf_score_reset(const gtf_score_state* state, gtf_stream_t stream);

/* Scratch of one gtf_score_candidates call (reconstruction_efficiency.py:125-134) over n_cand
 * candidates of n_members members in all (gtf_extract_out_counts: n_extracted,
 * n_extracted_nodes). Positive for zero sizes, non-decreasing in each argument (negative
 * counts as 0), depends on nothing else: no buffer is sized by the number of particle
 * entries, which has no bound the host knows (members need not be distinct). */
size_t gtf_score_workspace_bytes(int32_t n_cand, int32_t n_members);

/* reconstruction_efficiency.py:125-163 (gtf/metrics.py candidate_particles, majority and the
 * three tests of reconstruction_efficiency) for the candidates cand_ptr [n_cand + 1] (int32) /
 * cand_ids (int64 node ids), device arrays in gtf_extract_out's form; n_cand the host count
 * gtf_extract_outputs returned. The number of members is cand_ptr[n_cand], on the device: the
 * call takes the largest n_members with gtf_score_workspace_bytes(n_cand, n_members) <=
 * workspace_bytes as its capacity and sets GTF_SCORE_ERR_WORKSPACE (reading nothing past it)
 * when there are more.
 *   Per candidate, over the concatenation of its members' node_part rows (members in list
 * order, hits in node order): pid = the most frequent id, ties to the id whose first
 * occurrence comes first (Counter + max(key=get), :132-134), n_good its count, total the
 * number of entries; an empty candidate gives 0 / 0 / 0. It passes when pid is in part_id
 * with part_ref set, 2 n_good >= part_hits and 2 n_good >= total (:150-163, see above). A
 * passing candidate claims its particle with the key (group << 32) | index by a 64-bit
 * atomic minimum on that particle's own word, and in a second launch the candidate whose key
 * is the stored one writes best_good / best_total: its only writer. The smallest key wins, so
 * inside a call the first passing candidate (:166-171) and across calls the smallest group,
 * in whatever order the calls come: the reference reads iterations last, ..., 1 while the loop
 * produces 1, ..., last, so the caller passes group = last - iteration. Calls on one state
 * need distinct groups.
 *   Three launches and one hipCUB exclusive sum: the members' rows (a binary search each),
 * the vote (a 16-lane group per candidate of up to 16 entries, the wavefront for up to 64,
 * a whole-wave loop that is slow but correct for any length beyond), the winners. No atomic
 * on a shared word: the claims go to per-particle words and the error word is touched only
 * on a violation. Nothing is allocated, nothing synchronises. n_cand == 0: returns 0,
 * nothing launched. -3 for another ABI of *truth; -2 for a null truth / state / array that is
 * needed, negative sizes or group, state->n_particles != truth->n_particles, or a workspace
 * below gtf_score_workspace_bytes(n_cand, 0): all decided on the host before any launch. */
int gtf_score_candidates(const gtf_truth* truth, const int32_t* cand_ptr, const int64_t* cand_ids,
                         int32_t n_cand, int32_t group, const gtf_score_out* out,
                         const gtf_score_state* state, void* workspace, size_t workspace_bytes,
                         gtf_stream_t stream);

/* Scratch of gtf_score_finish (reconstruction_efficiency.py:166-171) for R region particles:
 * positive for 0, non-decreasing. */
size_t gtf_score_finish_workspace_bytes(int32_t n_particles);

/* reconstruction_efficiency.py:166-171, :213 (gtf/metrics.py: the match order of
 * reconstruction_efficiency): the matched particles, compacted and sorted by key (one hipCUB
 * radix sort of the R keys; the all-ones keys of the unmatched sort behind them), written as
 * n_reconstructed records in match order -- the order :166-171 appends the purities in:
 * out_key (the winning candidate's group and index), out_pid, out_good, out_total and
 * out_hits = part_hits, DEVICE arrays [R], NULL = not wanted. Synchronises `stream` once to
 * fill *counts. Returns -2 with "a candidate node has no hit_dissociation" when the error word
 * holds GTF_SCORE_ERR_MISSING (the reference's KeyError), -2 with their own messages for the
 * other two bits; -3 / -2 on the host before any launch as gtf_score_candidates. */
int gtf_score_finish(const gtf_truth* truth, const gtf_score_state* state, uint64_t* out_key,
                     int64_t* out_pid, int32_t* out_good, int32_t* out_total, int32_t* out_hits,
                     gtf_score_counts* counts, void* workspace, size_t workspace_bytes,
                     gtf_stream_t stream);

/* ---- Scoring a batch of events in one call: gtf_score_candidates_ev ------------------
 * reconstruction_efficiency.py:118-183 for the K events of a fused graph (gtf_graph_concat,
 * gtf_build_events_csr_device) at once: what K gtf_score_candidates / gtf_score_finish calls
 * compute, in launch sequences whose length does not depend on K. Node ids and particle ids of
 * different events collide (the same event twice is the plain case), so the K truth tables are
 * not merged: they lie end to end and every lookup stays inside its own event's segment, as
 * gtf_candidate_order_device_ev looks node ids up. gtf_score.hip.
 *
 * gtf_truth_batch: the K gtf_truth tables end to end, DEVICE arrays. node_id and part_id
 * ascend inside an event's segment only; node_ptr holds every event's pointers shifted by its
 * entry_off, and one closing entry. scored [K]: 0 = an event without truth, whose candidates are
 * not looked up, claim nothing, raise no GTF_SCORE_ERR_MISSING and get 0 / 0 / 0 / 0 in the
 * per-candidate outputs; NULL = every event is scored. */
typedef struct gtf_truth_batch {
    uint32_t struct_size;       /* sizeof(gtf_truth_batch) as the caller compiled it */
    uint32_t abi_version;       /* GTF_ABI_VERSION */
    int32_t n_events;           /* K */
    int32_t n_nodes;            /* sum of T, < 2^31 */
    int32_t n_entries;          /* sum of P, < 2^31 */
    int32_t n_particles;        /* sum of R, < 2^31 */
    const int32_t* node_off;    /* [K+1] event e's rows of node_id: node_off[e] .. node_off[e+1] */
    const int32_t* entry_off;   /* [K+1] ... of node_part */
    const int32_t* part_off;    /* [K+1] ... of part_id, part_hits, part_ref */
    const int64_t* node_id;     /* [sum T] */
    const int32_t* node_ptr;    /* [sum T + 1] */
    const int64_t* node_part;   /* [sum P] */
    const int64_t* part_id;     /* [sum R] */
    const int32_t* part_hits;   /* [sum R] */
    const uint8_t* part_ref;    /* [sum R] */
    const uint8_t* scored;      /* [K] or NULL */
} gtf_truth_batch;

/* One part of gtf_truth_concat: the sizes on the HOST (checked and summed before any launch) ... */
typedef struct gtf_truth_sizes {
    int32_t n_nodes, n_entries, n_particles, pad_;
} gtf_truth_sizes;

/* ... and the same sizes beside the part's arrays in a DEVICE table. A part of size 0 may hold
 * NULL arrays. */
typedef struct gtf_truth_part {
    int32_t n_nodes, n_entries, n_particles, pad_;
    const int64_t* node_id;
    const int32_t* node_ptr;
    const int64_t* node_part;
    const int64_t* part_id;
    const int32_t* part_hits;
    const uint8_t* part_ref;
} gtf_truth_part;

/* The caller-owned DEVICE arrays gtf_truth_concat fills, at the sizes of gtf_truth_batch. */
typedef struct gtf_truth_batch_buf {
    int32_t *node_off, *entry_off, *part_off;   /* each [K+1] */
    int64_t* node_id;
    int32_t* node_ptr;
    int64_t* node_part;
    int64_t* part_id;
    int32_t* part_hits;
    uint8_t* part_ref;
} gtf_truth_batch_buf;

/* Scratch of gtf_truth_concat: one word, set when the device table disagrees with the host's
 * sizes (rows are then left unwritten); positive for 0 parts. */
size_t gtf_truth_concat_workspace_bytes(int32_t n_parts);

/* gtf/metrics.py concat_tables on the device, with gtf_graph_concat's conventions: sizes
 * [n_parts] on the host, parts [n_parts] on the device. One block computes the three offset
 * arrays; one launch over nodes, entries and particles copies every row, a thread finding its
 * part by a binary search over the offsets (staged in LDS up to 2,048), node_ptr shifted by the
 * part's entry_off; every write is clamped to the host's sums. Two launches whatever n_parts
 * is; nothing synchronises, nothing is allocated. *out arrives with struct_size / abi_version
 * set and `scored` as the caller wants it, and leaves with the counts and buf's pointers.
 * Parts with T = 0, P = 0 or R = 0 are legal anywhere, and so is n_parts == 0. -3 for another
 * ABI of *out; -2 for a null argument or array that is needed, negative sizes, a sum of 2^31
 * or more, or a workspace below gtf_truth_concat_workspace_bytes: all before any launch. */
int gtf_truth_concat(const gtf_truth_sizes* sizes, const gtf_truth_part* parts, int32_t n_parts,
                     const gtf_truth_batch_buf* buf, gtf_truth_batch* out, void* workspace,
                     size_t workspace_bytes, gtf_stream_t stream);

/* gtf_score_state_ev: gtf_score_state for the whole batch, DEVICE arrays owned by the caller.
 * Event e's words are those of its own gtf_score_state, at part_off[e] on. */
typedef struct gtf_score_state_ev {
    uint32_t struct_size;       /* sizeof(gtf_score_state_ev) as the caller compiled it */
    uint32_t abi_version;       /* GTF_ABI_VERSION */
    int32_t n_particles;        /* sum of R of the gtf_truth_batch it is used with */
    int32_t pad_;
    uint64_t* best_key;         /* [sum R] (group << 32) | candidate index INSIDE ITS EVENT; all-ones = none */
    int32_t* best_good;         /* [sum R] */
    int32_t* best_total;        /* [sum R] */
    uint32_t* error;            /* [2] GTF_SCORE_ERR_* of all events; the smallest event index that set one
                                   (an atomic minimum that runs only on a violation), INT32_MAX = none */
} gtf_score_state_ev;

/* reconstruction_efficiency.py:118-121 per event. events == NULL: every key all-ones, the error
 * words cleared (0, INT32_MAX). Otherwise events is a DEVICE byte mask [K]: the keys of the
 * marked events alone are reset and the error words stay -- the reset of a scorer that holds
 * each event's latest iteration, where an event that has run out of nodes keeps its claims.
 * One launch, no synchronisation. -3 / -2 as gtf_score_candidates_ev. */
int gtf_score_reset_ev(const gtf_score_state_ev* state, const gtf_truth_batch* batch,
                       const uint8_t* events, gtf_stream_t stream);

/* Scratch of one gtf_score_candidates_ev call: as gtf_score_workspace_bytes, and one word per
 * candidate more (its event). Does not depend on n_events. */
size_t gtf_score_ev_workspace_bytes(int32_t n_cand, int32_t n_members, int32_t n_events);

/* gtf_score_candidates (reconstruction_efficiency.py:125-163) for the candidates of K events in
 * the form gtf_extract_outputs and gtf_event_split leave them for the fused graph: the global
 * cand_ptr [n_cand + 1] and cand_ids, not rebased, and cand_first [K + 1] (device): candidate c
 * belongs to the event e with cand_first[e] <= c < cand_first[e + 1], and so do its members.
 *   A small first launch finds every candidate's event (an upper bound over cand_first, staged
 * in LDS up to 2,048 entries) and checks cand_first; then the three launches and the exclusive
 * sum of gtf_score_candidates: a member is searched in node_id[node_off[e] .. node_off[e + 1]),
 * the vote is the same (16 lanes, the wavefront, the chunked loop), the particle is searched in
 * part_id[part_off[e] .. part_off[e + 1]) and claimed by a 64-bit atomic minimum on
 * best_key[part_off[e] + r] with the key (group << 32) | (c - cand_first[e]). After any sequence
 * of calls best_key, best_good and best_total are the K states of gtf_score_candidates laid end
 * to end, word for word, and the per-candidate outputs [n_cand] the K outputs concatenated.
 *   Nothing is allocated, nothing synchronises, no atomic on a shared word except on a
 * violation, every read is clamped to the batch's sums. cand_first[0] != 0, a decreasing
 * cand_first or cand_first[K] != n_cand set GTF_SCORE_ERR_RANGE and the candidates whose event
 * they leave open are skipped as those of an unscored event. More members than the workspace
 * holds: GTF_SCORE_ERR_WORKSPACE. n_cand == 0: returns 0, nothing launched. -3 for another ABI
 * of *batch or *state; -2 as gtf_score_candidates, before any launch. */
int gtf_score_candidates_ev(const gtf_truth_batch* batch, const int32_t* cand_ptr,
                            const int64_t* cand_ids, const int32_t* cand_first, int32_t n_cand,
                            int32_t group, const gtf_score_out* out, const gtf_score_state_ev* state,
                            void* workspace, size_t workspace_bytes, gtf_stream_t stream);

/* Scratch of gtf_score_finish_ev for sum R particles of K events: positive for 0, non-decreasing. */
size_t gtf_score_finish_ev_workspace_bytes(int32_t n_particles, int32_t n_events);

/* gtf_score_finish (reconstruction_efficiency.py:166-171, :213) per event: one hipCUB segmented
 * radix sort of the keys over part_off (which must be what gtf_truth_concat wrote), one count
 * per event, one exclusive sum, one launch that writes the records compacted: event e's at
 * rec_first[e] .. rec_first[e + 1] (rec_first: DEVICE [K + 1]), ascending by key inside the
 * event. out_*: DEVICE arrays [sum R], NULL = not wanted. n_reconstructed [K] and error [2] are
 * HOST arrays, filled by the call's one synchronisation. Errors return -2 with
 * gtf_score_finish's messages, led by the event of error[1] where there is one: "event 3: a
 * candidate node has no hit_dissociation". */
int gtf_score_finish_ev(const gtf_truth_batch* batch, const gtf_score_state_ev* state,
                        uint64_t* out_key, int64_t* out_pid, int32_t* out_good, int32_t* out_total,
                        int32_t* out_hits, int32_t* rec_first, int32_t* n_reconstructed,
                        uint32_t* error, void* workspace, size_t workspace_bytes,
                        gtf_stream_t stream);

/* ---- The truth tables themselves: gtf_truth_build ---------------------------------
 * gtf/metrics.py truth_tables (reconstruction_efficiency.py:41-91, helper.py:466-479) on the
 * device: from the parsed columns of the hit mapping, the truth file and the particles file,
 * DEVICE arrays in file row order, to the six arrays of a gtf_truth, array_equal to the host
 * function's. gtf_truth.hip.
 *
 * Limits. volume_id, layer_id and module_id of every mapping row must lie in [0, 2^21) (they
 * are packed into one sort key; TrackML uses at most 18, 14 and about 3,200): checked on the
 * device, GTF_TRUTH_ERR_RANGE. Node, hit and particle ids are arbitrary int64 (0, negative and
 * 60-bit ids included). Each of n_rows, n_truth and n_particles is at most 2^30. */
typedef struct gtf_truth_in {
    uint32_t struct_size;        /* sizeof(gtf_truth_in) as the caller compiled it */
    uint32_t abi_version;        /* GTF_ABI_VERSION */
    int32_t n_rows;              /* rows of the mapping */
    int32_t n_truth;             /* rows of the truth columns; 0 = the mapping's own hit_id / particle_id */
    int32_t n_particles;         /* rows of the particles table */
    int32_t num_layers;          /* distinct (volume, layer) a reference track needs (:66: 4) */
    int32_t min_volume;          /* the region: min_volume <= volume_id <= max_volume */
    int32_t max_volume;
    double pt_cut;               /* sqrt(px*px + py*py) >= pt_cut in fp64 (:46: 1.0) */
    const int64_t* node_idx;     /* [n_rows] the six columns of the mapping */
    const int64_t* hit_id;
    const int64_t* particle_id;
    const int64_t* volume_id;
    const int64_t* layer_id;
    const int64_t* module_id;
    const int64_t* truth_hit;    /* [n_truth] or NULL with n_truth == 0 */
    const int64_t* truth_part;
    const int64_t* part_id;      /* [n_particles] */
    const double* px;            /* [n_particles] */
    const double* py;
} gtf_truth_in;

/* The caller's output arrays at their bound: T, P and R are each at most n_rows. */
typedef struct gtf_truth_buf {
    int64_t* node_id;            /* [n_rows] */
    int32_t* node_ptr;           /* [n_rows + 1] */
    int64_t* node_part;          /* [n_rows] */
    int64_t* part_id;            /* [n_rows] */
    int32_t* part_hits;          /* [n_rows] */
    uint8_t* part_ref;           /* [n_rows] */
} gtf_truth_buf;

#define GTF_TRUTH_ERR_MISSING 1u   /* a mapped hit has no truth row (the host's ValueError) */
#define GTF_TRUTH_ERR_RANGE   2u   /* a volume_id, layer_id or module_id outside [0, 2^21) */

typedef struct gtf_truth_counts {
    int32_t n_nodes;             /* T */
    int32_t n_entries;           /* P */
    int32_t n_particles;         /* R */
    int32_t n_reference;         /* the sum of part_ref */
    uint32_t error;              /* GTF_TRUTH_ERR_* */
    int32_t pad_;
} gtf_truth_counts;

/* Scratch of gtf_truth_build: positive for zero sizes, non-decreasing in each argument (negative
 * counts as 0; n_truth == 0 counts as n_rows). About 130 bytes per row at n_truth == n_rows. */
size_t gtf_truth_build_workspace_bytes(int32_t n_rows, int32_t n_truth, int32_t n_particles);

/* metrics.truth_tables line by line:
 *   - a particle is high-pT when sqrt(px*px + py*py) >= pt_cut, in fp64 with NumPy's roundings;
 *   - a mapping row is in the region when its volume lies in the window and its hit_id has at
 *     least one truth row whose particle is high-pT (np.isin over hits: a row can be selected
 *     through another row of its hit; with separate truth columns the mapping's own
 *     particle_id plays no part in the selection);
 *   - part_id: the distinct particle_id of the region rows, ascending as signed int64;
 *     part_hits their region rows (repeated rows count); part_ref = 1 with at least num_layers
 *     distinct (volume, layer) and no (volume, layer, module) twice among the particle's rows;
 *   - node_id / node_ptr / node_part: the first row of every distinct (node_idx, hit_id) pair,
 *     grouped by ascending node, a node's entries in mapping-row order; each entry the particle
 *     of the FIRST truth row, in row order, with that hit id.
 * Six hipCUB radix sorts (particles, truth rows by hit, rows by packed module key and by
 * particle, rows by node and by hit), exclusive sums of packed marks, binary searches; no atomic
 * but the error word's on a violation. Nothing is allocated. Synchronises `stream` once, to fill
 * *counts; *out then holds buf's pointers and the counts, ready for gtf_score_candidates.
 * Nothing is written past node_id[T], node_ptr[T + 1], node_part[P], part_*[R].
 * Returns -2 with GTF_TRUTH_ERR_MISSING or GTF_TRUTH_ERR_RANGE in counts->error (the arrays are
 * then unspecified); -3 for another ABI of *in; -2 for a null argument or array that is needed,
 * negative sizes, more than 2^30 rows, min_volume > max_volume or a small workspace, all
 * decided on the host before any launch. n_rows == 0: returns 0 with zero counts and
 * node_ptr[0] = 0 (one stream-ordered fill), nothing else written, no workspace needed. */
int gtf_truth_build(const gtf_truth_in* in, const gtf_truth_buf* buf, gtf_truth* out,
                    gtf_truth_counts* counts, void* workspace, size_t workspace_bytes,
                    gtf_stream_t stream);

/* ---- A batch's truth tables in one call: gtf_truth_build_ev ----------------------------
 * gtf/metrics.py truth_tables_batch (reconstruction_efficiency.py:41-91, helper.py:466-479 per
 * event) on the device: the parsed columns of K events laid end to end go in, and what comes
 * out is the gtf_truth_batch that gtf_truth_concat of the K single gtf_truth_build results
 * leaves, word for word. gtf_truth.hip.
 *
 * One window and one cut per batch. Event e's mapping rows are row_off[e] .. row_off[e + 1]
 * of the six mapping columns, its truth rows truth_off[e] .. truth_off[e + 1] of truth_hit /
 * truth_part, its particles particle_off[e] .. particle_off[e + 1] of part_id / px / py. The
 * three offset arrays are HOST arrays of n_events + 1 int32, start at 0 and do not decrease.
 * An event with truth_off[e] == truth_off[e + 1] and rows uses its mapping's own hit_id /
 * particle_id as truth columns (gtf_truth_in's n_truth == 0); both kinds may be mixed. The
 * limits of gtf_truth_build hold for the sums. */
typedef struct gtf_truth_in_ev {
    uint32_t struct_size;        /* sizeof(gtf_truth_in_ev) as the caller compiled it */
    uint32_t abi_version;        /* GTF_ABI_VERSION */
    int32_t n_events;            /* K */
    int32_t num_layers;          /* as gtf_truth_in */
    int32_t min_volume;
    int32_t max_volume;
    double pt_cut;
    const int32_t* row_off;      /* HOST [K + 1] */
    const int32_t* truth_off;    /* HOST [K + 1] */
    const int32_t* particle_off; /* HOST [K + 1] */
    const int64_t* node_idx;     /* DEVICE [row_off[K]] the six columns of the mappings */
    const int64_t* hit_id;
    const int64_t* particle_id;
    const int64_t* volume_id;
    const int64_t* layer_id;
    const int64_t* module_id;
    const int64_t* truth_hit;    /* DEVICE [truth_off[K]] or NULL when that is 0 */
    const int64_t* truth_part;
    const int64_t* part_id;      /* DEVICE [particle_off[K]] */
    const double* px;
    const double* py;
} gtf_truth_in_ev;

/* Scratch of gtf_truth_build_ev for the summed sizes: positive for zero sizes, non-decreasing in
 * each argument (negative counts as 0). The truth tables are sized for n_rows + n_truth rows, so
 * it does not depend on which events bring truth columns of their own. */
size_t gtf_truth_build_ev_workspace_bytes(int32_t n_rows, int32_t n_truth, int32_t n_particles,
                                          int32_t n_events);

/* gtf_truth_build's five steps (reconstruction_efficiency.py:41-91, helper.py:466-479) on global
 * indices. A first launch writes one int32 event column per axis (a binary search over the
 * offsets, uploaded once in stream order). Ids of different events collide and cannot be
 * shifted, so every sorted table is ordered by (event, key): the 64-bit key sort, then one
 * stable radix pass over the bits K needs on the event word (skipped at K == 1). Every lookup
 * stays inside its event's segment, heads also break at an event boundary, and the three
 * offset arrays are the existing exclusive sums read at row_off[e]. node_ptr holds global entry
 * indices and one closing entry.
 *   buf: the arrays at their bounds: row_off[K] rows (+ 1 for node_ptr), K + 1 per offset array.
 * *out arrives with struct_size, abi_version and scored set, as for gtf_truth_concat, and leaves
 * with the sums and buf's pointers. counts: a HOST array [K]; counts[e].error holds event e's
 * GTF_TRUTH_ERR_* bits (one device word per event, touched only on a violation). A number of
 * launches that does not depend on K, one synchronisation, nothing allocated. Nothing is
 * written past node_id[sum T], node_ptr[sum T + 1], node_part[sum P], part_*[sum R] or an offset
 * array's K + 1.
 *   Returns -2 with the smallest failing event named: "event 3: a mapped hit has no truth row",
 * "event 3: a volume_id, layer_id or module_id outside [0, 2^21)" (the arrays are then
 * unspecified). -3 for another ABI of *in or *out; -2 for a null argument or array that is
 * needed, a negative n_events, an offset array that does not start at 0 or decreases, a sum
 * above 2^30 rows, min_volume > max_volume or a small workspace: all before any launch.
 * K == 0 and events without rows, particles or truth rows are legal anywhere; with no rows at
 * all the call writes the three zero offset arrays and node_ptr[0] = 0 and returns without a
 * synchronisation (no column and no workspace needed). */
int gtf_truth_build_ev(const gtf_truth_in_ev* in, const gtf_truth_batch_buf* buf, gtf_truth_batch* out,
                       gtf_truth_counts* counts, void* workspace, size_t workspace_bytes,
                       gtf_stream_t stream);

/* ---- Parabolic-model KL training data -------------------------
 * learn_KL_parabolic_model/src/generate_training_data: the per-edge parabolic
 * state of compute_track_state_estimates (utils.py:221-289; S = diag(16, 0.01,
 * 0.01), H rows [x^2, x, 1]) for every in-edge of a node, and the pairwise KL
 * distance KLDistance / calc_pairwise_distances (extract_metadata_trackml_parabolic_
 * model.py:15-25) of every pair i > j of a node with >= 2 in-edges (:61-62), with the
 * node's gradient variance (utils.py:240-254, :286) and the pair truth flag (:82-95).
 *
 * Pairs of node v are written at out->kl[pair_ptr[v] + t], t = i (i - 1) / 2 + j
 * (row-major lower triangle over the node's in-slots, slot order); pair_ptr[v + 1] -
 * pair_ptr[v] must be d (d - 1) / 2 for d = slot_ptr[v + 1] - slot_ptr[v] >= 2, else 0.
 * emp_var is the variance over in-neighbours, which is the reference's variance
 * over nx.all_neighbors when the edge set is symmetric (helper.py:512-518 adds both
 * directions). */
typedef struct gtf_kl_graph {
    int32_t n_nodes, n_slots;
    const int32_t* slot_ptr;  /* [N+1] in-edge CSR (every slot an edge) */
    const int32_t* slot_src;  /* [S] neighbour of each in-edge */
    const double* gnn;        /* [N*gnn_stride] GNN_Measurement x, y(, z, r) */
    const int64_t* truth;     /* [N] truth_particle, or NULL */
    const int64_t* pair_ptr;  /* [N+1] */
    const int32_t* list[4];   /* nodes to process by in-degree bucket, any order within a bucket:
                                 d in [1, 2], [3, 4] (one thread each), [5, 8] (8-lane groups) and d > 8
                                 (one 64-lane wavefront each); d = 1 nodes yield states and
                                 gradient moments but no pairs */
    int32_t count[4];
    /* ordered layout (v3; gtf.parabolic.ParabolicKL(ordered=True)): when every list[i] is
     * NULL, bucket i is the node range [first[i], first[i] + count[i]), and bucket 0 holds
     * n_d1 one-edge nodes, then its two-edge nodes, with consecutive slots from slot0 (in
     * node order) and one pair each from pair0: the kernel then reaches bucket 0's slots,
     * neighbours and pairs by arithmetic, and every bucket's nodes without a list load. */
    int32_t first[4];
    int32_t n_d1;
    int32_t gnn_stride;       /* doubles per gnn row: 0 or 4 (x, y, z, r), or 2 (a compact x, y copy:
                                 the kernel reads only x and y, so half the gathered bytes) */
    int64_t slot0;
    int64_t pair0;
    /* tiled layout (gtf.parabolic.ParabolicKL(tile=T)): the nodes azimuth-sorted per event and
     * cut into tiles of <= 256 one- / two-edge (bucket-0) nodes and the nodes between them, bucket
     * 0 first inside a tile (one-edge, then two-edge nodes, consecutive slots and one pair each).
     * One 256-thread block per tile record of 12 int32: (first node, bucket-0 count n0, its
     * one-edge count, the in-tile three-edge count n3, the in-tile four-edge count n4, 0, bucket
     * 0's first slot, its first pair low / high 32 bits, window [lo, hi) of at most 1024
     * consecutive nodes holding the tile's neighbours, 0); the n3 three-edge and then n4
     * four-edge nodes follow the tile's bucket-0 nodes (slots and pairs consecutive) and run in
     * the tile's block, one thread per node, so n0 + n3 + n4 <= 256 (the block skips nodes past
     * 256 without an error; gtf.parabolic.ParabolicKL._block_table refuses such tiles). n3 and
     * n4 must be 0 when list[1] is given (bucket 1 then runs by list). The block loads its
     * sender lists and the window's x, y and truth ids in one round and reads the neighbours from
     * LDS. Buckets 1..3 come from list[1..3] / count[1..3] (count[0] and list[0] are ignored). The
     * library clamps each window to its LDS size but does not check the records' node, slot and
     * pair ranges against the arrays (they live in device memory): build them with
     * gtf.parabolic.ParabolicKL(tile=T), or keep every range inside n_nodes / n_slots. */
    const int32_t* blk;       /* [12 * n_blk] or NULL */
    int32_t n_blk;
    /* ordered layout, degree runs (round 4): deg_runs = 1 when buckets 1 and 2 hold their nodes
     * sorted by in-degree, n_deg[k] nodes of in-degree 3 + k (k = 0..5) one run after another
     * (sum n_deg[0..1] = count[1], sum n_deg[2..5] = count[2]), with consecutive slots and pairs
     * after bucket 0's: the kernel then finds their slots and pairs by arithmetic as well (one
     * dependent round of loads fewer). 0: slot_ptr / pair_ptr are read per node. */
    int32_t deg_runs;
    int32_t n_deg[6];
    int32_t pad_deg_;
} gtf_kl_graph;

enum { GTF_F64 = 0, GTF_F32 = 1 };

typedef struct gtf_kl_out {
    void* kl;          /* [P] double (GTF_F64) or float (GTF_F32) */
    int8_t* truth;     /* [P] or NULL (needs graph truth) */
    double* emp_var;   /* [N] or NULL; np.var of the gradients, written for the listed nodes */
    double* emp_mean;  /* [N] or NULL; np.mean of the gradients (xy_edge_gradient_mean_var[0]) */
    double* sv;        /* [S*3] edge_state_vector or NULL */
    double* cov;       /* [S*9] edge_covariance (row-major) or NULL */
    uint32_t* err;     /* device error word (GTF_ERR_SINGULAR_H) or NULL */
} gtf_kl_out;

/* dtype: GTF_F64 computes states and distances in fp64 (the reference's precision);
 * GTF_F32 rotates/translates in fp64 and forms states and distances in fp32 (the
 * config-5 tolerance sweep). sv/cov outputs are fp64 in both modes.
 *
 * GTF_ERR_SINGULAR_H. The flag is geometric: it is raised for an in-edge of a listed node whose
 * x_B == 0, x_B == x_0 or x_0 == 0, compared on the fp64 values of the kernel's own rotation
 * (cos, sin = x / h, -y / h; gtf_parabolic_kl_q32: on its fp32 values from the fixed-point
 * coordinates). That is wherever the reference raises LinAlgError (utils.py:285 on H, or the
 * script's own np.linalg.inv of the garbage covariance, :78), and additionally at exact geometric
 * singularity where the reference does not raise: rotating by cos / sin(2 pi - atan2) leaves it a
 * pivot of a few ulp there and it returns unbounded values (covariance entries of 1e14 to 1e28),
 * e.g. node (10, 0) with neighbour (10, 5), or any node with a neighbour at the origin. The
 * record of both behaviours, image by image, is tests/golden/kl_cases.npz (tests/kl_cases.py).
 * The raising edge's state and its pairs are not finite; every other output of the call is
 * written as usual. */
int gtf_parabolic_kl(const gtf_kl_graph* g, int32_t dtype, const gtf_kl_out* out, gtf_stream_t stream);

/* Compact input mode (gtf.parabolic.ParabolicKL(compact=True)): the same states, distances,
 * gradient moments and truth flags (utils.py:221-289) from 32-bit fixed-point coordinates
 * and int32 truth ids -- 12 bytes per node where gtf_kl_graph's fp64 x, y and int64 id take
 * 24 -- computed in fp32 throughout.
 * Quantisation rule (gtf.parabolic.quantise_xy): scale = 2^(e - 30) with e the smallest
 * integer such that every |x|, |y| < 2^e, and q = rint(x / scale), so every |q| < 2^30 and
 * q * scale is within scale / 2 of x. |q| < 2^30 is REQUIRED of the caller (it is not
 * checked: the coordinates live in device memory): the difference of two coordinates then
 * fits an int32 exactly, so the kernel translates a neighbour to its node in integers with
 * no rounding and only the differences, not the coordinates, are rounded to fp32. (Plain
 * fp32 coordinates lose that: their rounding alone costs the fp32 mode's error bar.) */
typedef struct gtf_kl_q32 {
    const int32_t* xy;       /* [N*2] (qx, qy) per node, 8-byte aligned; x = qx * scale, y = qy * scale */
    double scale;            /* finite, > 0; a power of two by the rule above */
    const int32_t* truth32;  /* [N] truth_particle, or NULL */
} gtf_kl_q32;

typedef struct gtf_kl_out32 {
    float* kl;         /* [P] */
    int8_t* truth;     /* [P] or NULL (needs q->truth32) */
    float* emp_var;    /* [N] or NULL; np.var of the gradients dqy / dqx, summed in fp64, stored as float */
    float* emp_mean;   /* [N] or NULL; np.mean of the gradients */
    uint32_t* err;     /* device error word (GTF_ERR_SINGULAR_H) or NULL */
} gtf_kl_out32;        /* (no sv / cov: full states are an fp64 service of gtf_parabolic_kl) */

/* g supplies the structure only -- the CSR, pair_ptr, the lists or the ordered / degree-run
 * fields, blk -- in any of gtf_kl_graph's three layouts; g->gnn, g->gnn_stride and g->truth
 * are ignored. Pairs, moments and the error word are laid out as gtf_parabolic_kl's. */
int gtf_parabolic_kl_q32(const gtf_kl_graph* g, const gtf_kl_q32* q, const gtf_kl_out32* out, gtf_stream_t stream);

/* ---- The KL graph itself: gtf_kl_prepare -----------------------------------------------
 * gtf/parabolic.py ParabolicKL.__init__ with tile = 0 (lines 154-278) on the device: from a
 * slot CSR, the coordinates and the truth ids, DEVICE arrays in the caller's order, to every
 * array a gtf_kl_graph / gtf_kl_q32 points to, equal element for element to what the
 * constructor uploads. That constructor restates the input side of the reference's
 * learn_KL_parabolic_model/src/generate_training_data (extract_metadata_trackml_parabolic_
 * model.py:15-99: the in-edges of every node, their pairs i > j; utils.py:221-289 reads x, y);
 * the orders and the fixed-point copy are this project's own. gtf_kl_prepare.hip. */
typedef struct gtf_kl_prepare_in {
    uint32_t struct_size;      /* sizeof(gtf_kl_prepare_in) as the caller compiled it */
    uint32_t abi_version;      /* GTF_ABI_VERSION */
    int32_t n_nodes, n_slots;  /* N, S: each at most 2^30 */
    const int32_t* slot_ptr;   /* [N+1] starts at 0, does not decrease, ends at S (checked on the device) */
    const int32_t* slot_src;   /* [S] sender of each slot; a kept slot's lies in [0, N) (checked on the device) */
    const uint8_t* is_edge;    /* [S] or NULL = every slot is an edge. Non-zero: the slot is kept, in slot order
                                  (parabolic.py:66-75 in_edge_csr); a dropped slot's slot_src is never read */
    const double* gnn;         /* [N*gnn_stride] x, y(, z, r) in the caller's node order */
    const int64_t* truth;      /* [N] truth_particle, or NULL */
    int32_t gnn_stride;        /* 2 or 4 */
    int32_t with_single;       /* one-edge nodes are listed (parabolic.py:174 lo = 1) */
    int32_t layout;            /* 0 natural (bucket lists, :219, :261-265), 1 ordered with degree runs (:178-184, :199-213, :249-260) */
    int32_t compact;           /* also the fixed-point coordinates and int32 truth ids (:267-278) */
    double scale;              /* compact: 0 = derive (quantise_xy, :51-56), else used as it is */
} gtf_kl_prepare_in;

/* The caller's output arrays. Those a call does not need may be NULL. */
typedef struct gtf_kl_prepare_buf {
    int32_t* slot_ptr;         /* [N+1] */
    int32_t* slot_src;         /* [S]; the first `kept slots` are written */
    double* xy;                /* [N*2] */
    int64_t* truth;            /* [N] with in.truth */
    int64_t* pair_ptr;         /* [N+1] exclusive sum of d (d - 1) / 2 for d >= 2, else 0 (:215-217) */
    int32_t* list;             /* [N] layout 0: the four bucket lists one after another, each ascending (:219);
                                  the words after the n_listed-th are unspecified */
    int64_t* node_of;          /* [N] layout 1: the stable argsort of the degree rank (:199, :212) */
    int64_t* slot_of;          /* [S] layout 1: the in-edge CSR's slot of every new slot (:204) */
    int32_t* q;                /* [N*2] compact: rint(x / scale) (:60-63), 8-byte aligned */
    int32_t* truth32;          /* [N] compact with in.truth: the id where every id lies in [-2^31, 2^31), else its
                                  rank among the sorted distinct signed ids (np.unique's inverse, :274-277) */
} gtf_kl_prepare_buf;

#define GTF_KL_ERR_SLOT_PTR  1u   /* slot_ptr does not start at 0, decreases or does not end at n_slots */
#define GTF_KL_ERR_SOURCE    2u   /* a kept slot's source outside [0, N) */
#define GTF_KL_ERR_NONFINITE 4u   /* compact: a NaN or inf coordinate (quantise_xy's ValueError, :49-50) */
#define GTF_KL_ERR_FIT       8u   /* compact: some |q| >= 2^30 under the given scale (:61-62) */
#define GTF_KL_ERR_SCALE     16u  /* compact: the derived scale is not finite and > 0 (:58-59) */
#define GTF_KL_ERR_NODE_OF   32u  /* gtf_kl_coords: a node_of entry outside [0, N) */

typedef struct gtf_kl_counts {
    int32_t n_kept;            /* kept slots: the graph's n_slots */
    int32_t n_listed;          /* nodes in the four buckets (:220) */
    int64_t n_pairs;           /* pair_ptr[N] */
    int32_t count[4];          /* gtf_kl_graph.count */
    int32_t first[4];          /* gtf_kl_graph.first (layout 0: zero; list q starts at the sum of the counts before it) */
    int32_t n_d1;
    int32_t n_deg[6];
    uint32_t error;            /* GTF_KL_ERR_* */
    double scale;              /* compact: the scale used */
    double max_abs;            /* compact: the largest finite |x|, |y| */
} gtf_kl_counts;

/* Scratch of gtf_kl_prepare: positive for zero sizes, non-decreasing in each argument (negative
 * counts as 0). About 70 bytes per node and 12 per slot. */
size_t gtf_kl_prepare_workspace_bytes(int32_t n_nodes, int32_t n_slots);

/* ParabolicKL.__init__ line by line:
 *   - with is_edge the kept slots in slot order and their slot_ptr (in_edge_csr);
 *   - layout 1: rank = the first true key of [d == 1 if with_single] + [d == q for q in 2..8] +
 *     [d > 8], 9 for unlisted nodes (:181-184); node_of = its stable argsort (:199), ONE stable
 *     4-bit hipCUB radix pass; slot_ptr, slot_of, slot_src through the inverse order, x, y and
 *     truth permuted (:200-211); count, first, n_d1, n_deg, deg_runs = 1 (:250-260);
 *   - layout 0: the arrays in the caller's order and the bucket lists (:219), the same radix pass
 *     on the bucket number; an empty list is NULL in *out;
 *   - compact: one reduction for the largest |x|, |y|; scale = 2^(e - 30) with quantise_xy's
 *     e += 1 step, e = 0 for all-zero input; q = rint(x / scale), ties to even. The scale stays
 *     on the device for the quantising launch and comes back with the counts. The 64-bit sort of
 *     the truth ids always runs and the writing kernel chooses by a device flag whether it
 *     stores the ids or their ranks: ONE synchronisation, to fill *counts.
 * The number of launches does not depend on N. No atomic but the error word's on a violation.
 * Nothing is allocated. *out (gnn_stride 2, slot0 = pair0 = 0, no blk) and, with compact, *q32
 * hold buf's pointers and the counts, ready for gtf_parabolic_kl / gtf_parabolic_kl_q32.
 * Returns -2 with GTF_KL_ERR_* in counts->error and gtf_last_error() naming the rule (the
 * arrays are then unspecified; nothing is written outside them); -3 for another ABI of *in; -2
 * before any launch for a null argument or array that is needed, negative sizes, more than 2^30
 * nodes or slots, another gnn_stride or layout, a negative or non-finite scale or a small
 * workspace. N == 0 (then S == 0): slot_ptr[0] = pair_ptr[0] = 0 by two stream-ordered fills,
 * no workspace needed. S == 0 is legal. */
int gtf_kl_prepare(const gtf_kl_prepare_in* in, const gtf_kl_prepare_buf* buf, gtf_kl_graph* out, gtf_kl_q32* q32,
                   gtf_kl_counts* counts, void* workspace, size_t workspace_bytes, gtf_stream_t stream);

/* The coordinate step alone (parabolic.py:468-471 and :269, ParabolicKL.replica): gnn in the
 * caller's node order, node_of [N] or NULL (identity); writes xy [N*2] and / or q [N*2] with the
 * GIVEN scale, each NULL or written, by gtf_kl_prepare's own kernel. Stream-ordered, no
 * synchronisation: GTF_KL_ERR_NONFINITE / _FIT / _NODE_OF are or-ed into the device word *err
 * (required), which the caller clears and reads. */
int gtf_kl_coords(int32_t n_nodes, const double* gnn, int32_t gnn_stride, const int64_t* node_of, double* xy, int32_t* q,
                  double scale, uint32_t* err, gtf_stream_t stream);

/* The columns of the training rows (parabolic.py:559-571 pair_index and the emp_var[node] gather
 * of training_rows_csr, :609-610; extract_metadata_trackml_parabolic_model.py:61-99 writes one
 * row per pair): for pair row p of node v (pair_ptr[v] <= p < pair_ptr[v + 1]; nodes without
 * pairs are passed over), t = p - pair_ptr[v]: node[p] = node_of[v] (v with node_of NULL), i[p]
 * the integer with i (i - 1) / 2 <= t < (i + 1) i / 2, j[p] = t - i (i - 1) / 2, emp_row[p] =
 * emp_var[v] (dtype GTF_F64: double, GTF_F32: float; both NULL: no such column). g supplies
 * n_nodes, pair_ptr and slot_ptr; n_pairs = pair_ptr[N]. Stream-ordered. */
int gtf_kl_pair_rows(const gtf_kl_graph* g, int64_t n_pairs, const int64_t* node_of, const void* emp_var, int32_t dtype,
                     int64_t* node, int64_t* i, int64_t* j, void* emp_row, gtf_stream_t stream);

/* ---- event conversion: CSV rows -> packed CSR in the reference's orders -------------
 * Replaces helper.construct_graph + nx.DiGraph + the weakly-connected-component
 * subgraph copies of event_conversion.py:63-84 (helper.py:465-521) and the key order of
 * helper.compute_track_state_estimates' dicts (helper.py:277, 350-351). Host function
 * (no device work): the packed graph then goes to the GPU, where
 * gtf_track_state_estimates and gtf_node_ops compute the states, priors, mixture
 * weights and degrees. Orders are CPython 3.10 set orders, reproduced exactly. */
typedef struct gtf_event_csr {
    int64_t n_nodes;          /* in: nodes kept by the volume window, CSV order */
    int64_t n_rows;           /* in: edges.csv rows */
    const int64_t* node_id;   /* in: [n_nodes] node_idx, unique, in [0, 2^61 - 1) */
    const int64_t* row_a;     /* in: [n_rows] second column (node1): add_edge(a, b) first */
    const int64_t* row_b;     /* in: [n_rows] first column (node2) */
    int32_t* order;           /* out: [n_nodes] CSV index of packed node i */
    int32_t* sub_id;          /* out: [n_nodes] subgraph (weakly connected component) */
    int32_t* slot_ptr;        /* out: [n_nodes + 1] */
    int32_t* slot_src;        /* out: [2 * n_rows] packed sender per slot (ascending per receiver) */
    int32_t* tse_rank;        /* out: [2 * n_rows] track_state_estimates dict position */
    int32_t* out_ptr;         /* out: [n_nodes + 1] */
    int32_t* out_slot;        /* out: [2 * n_rows] successor order */
    int64_t n_edges;          /* out: directed edges (= slots) */
    int32_t n_subgraphs;      /* out */
    int32_t pad_;
} gtf_event_csr;

int gtf_build_event_csr(gtf_event_csr* ev);

/* The same build on the GPU (SURVEY §8f #2 "graph build on device"; gtf_build_dev.hip):
 * every pointer of `ev` a DEVICE array of the sizes above, the outputs equal to
 * gtf_build_event_csr's bit for bit (radix sorts for the id lookup and networkx's
 * successor insertion order, hook + pointer jumping for the weakly connected components,
 * CPython 3.10 set tables in the workspace for the set orders). Synchronises `stream`
 * (n_edges / n_subgraphs are returned in `ev`). Replaces helper.construct_graph
 * (helper.py:465-521) and event_conversion.py:63-84 like the host builder. */
size_t gtf_build_event_device_workspace_bytes(int64_t n_nodes, int64_t n_rows);
int gtf_build_event_csr_device(gtf_event_csr* ev, void* workspace, size_t workspace_bytes, gtf_stream_t stream);

/* A batch of K events in ONE build (gtf_build_dev.hip): replaces running event_conversion.py
 * (:53-101; helper.construct_graph, helper.py:465-521) once per event and fusing the results
 * (gtf/graph.py concat). *ev is gtf_event_csr with the events' columns laid end to end in
 * event order -- n_nodes = N and n_rows = R the sums, node_id / row_a / row_b and the seven
 * outputs DEVICE arrays at the summed sizes -- and *b says where each event starts. The result
 * is gtf_build_event_csr of every event, shifted by the sizes of the events before it as
 * gtf_graph_concat shifts: order and slot_src by the nodes before, sub_id by the subgraphs,
 * slot_ptr and out_slot by the slots, out_ptr by the edges, tse_rank as it is; n_edges and
 * n_subgraphs are the batch's. Node ids are looked up inside their own event: the same id
 * (the same event twice) may appear in any number of events, a row end that its own event
 * does not hold drops the row even if another event holds that id, a repeated id is an error
 * inside one event only (the message names the first such event), and the 2|c| >= |G| rule
 * of the node order counts the nodes of the component's own event. Event e's packed nodes
 * are the positions [node_off[e], node_off[e+1]). Events without nodes, without rows, or
 * with rows that are all dropped are legal anywhere.
 * Synchronises `stream` as often as gtf_build_event_csr_device does for one event: the count
 * does not grow with K, and the component rounds are the deepest event's, not their sum. */
typedef struct gtf_event_batch {
    uint32_t struct_size;      /* sizeof(gtf_event_batch) as the caller compiled it */
    uint32_t abi_version;      /* GTF_ABI_VERSION */
    int32_t n_events;          /* K >= 0 */
    int32_t pad_;
    const int32_t* node_off;   /* HOST [K+1]: event e's nodes are [node_off[e], node_off[e+1]); 0 first, N last */
    const int32_t* row_off;    /* HOST [K+1]: the same for the edge rows; 0 first, R last */
    int32_t* event;            /* out, DEVICE [N] or NULL: the event of every packed node */
} gtf_event_batch;

/* includes the two offset tables, which the call uploads; non-decreasing in every argument */
size_t gtf_build_events_device_workspace_bytes(int64_t n_nodes, int64_t n_rows, int32_t n_events);

/* -3: *b built against another layout of this header (struct_size, abi_version).
 * -2, decided on the host before any launch: a NULL ev, b, offset table, workspace or array
 * that the sizes need; offsets that do not start at 0, decrease, or end elsewhere than at
 * n_nodes / n_rows; n_nodes or 2 * n_rows above INT32_MAX / 2; a workspace below
 * gtf_build_events_device_workspace_bytes. -2 after the first synchronisation: a node id
 * outside [0, 2^61 - 1), a repeated id inside one event. The kernels of this call clamp every
 * write to the outputs' sizes. */
int gtf_build_events_csr_device(gtf_event_csr* ev, const gtf_event_batch* b, void* workspace, size_t workspace_bytes,
                                gtf_stream_t stream);

/* ---- event conversion: the packed event's columns and empty states, on the GPU --------
 * What is left of event conversion between the CSR above and gtf_track_state_estimates:
 * the node attributes construct_graph stores (helper.py:465-545: GNN_Measurement, xyzr,
 * in_volume_layer_id, vivl_id) in packed node order, and the arrays of an event that holds
 * no state yet (event_conversion.py:53-101: every edge activated, every node with an empty
 * track_state_estimates dict) -- array for array gtf/io.py build_event_csr. gtf_event.hip.
 *
 * A C caller's sequence from CSV columns to iteration 1: upload the columns,
 * gtf_build_event_csr_device, allocate at the returned n_edges, gtf_event_pack,
 * gtf_fill_columns (once per axis), gtf_graph_prepare, gtf_track_state_estimates,
 * gtf_node_ops (priors_tse, mw_tse, degree), gtf_refresh_send_mw. */

/* gtf_event_cols: the CSV columns of the kept nodes (helper.py:524-531), DEVICE arrays in
 * CSV row order -- the rows ev->node_id names. r stays an input: the reference computes it
 * with the C library's pow (helper.py:12-13; gtf/io.py edge_length_xy), which is the CSV
 * reader's business. layer_id must be >= 0 (the volume window's lower bound). */
typedef struct gtf_event_cols {
    const double* x;           /* [n_nodes] */
    const double* y;           /* [n_nodes] */
    const double* z;           /* [n_nodes] */
    const double* r;           /* [n_nodes] */
    const int64_t* layer_id;   /* [n_nodes] */
} gtf_event_cols;

/* gtf_event_out: the node attributes of helper.py:465-545 as DEVICE arrays in packed node
 * order (N = ev->n_nodes), caller-allocated; NULL = not wanted. */
typedef struct gtf_event_out {
    double*  gnn;       /* [N*4] (x, y, z, r)[order]: gtf_graph.gnn */
    double*  xyzr;      /* [N*4] the same bits, a separate array: gtf_graph.xyzr */
    double*  layer;     /* [N]   (double)(layer_id % 100): gtf_graph.layer */
    int64_t* node_id;   /* [N]   ev->node_id[order] */
    double*  vivl;      /* [N*2] (layer_id / 1000, layer_id % 100), integer division: gtf_extract_io.vivl */
    uint8_t* solo;      /* [N]   1 = alone in its subgraph: gtf_graph.solo */
} gtf_event_out;

/* After gtf_build_event_csr_device on the same device *ev (event_conversion.py:53-101,
 * helper.py:465-545): reads ev->n_nodes, order, node_id and sub_id (non-decreasing in packed
 * order, as the builder leaves it: solo compares the two neighbouring entries) and the
 * columns of *in; writes the wanted arrays of *out on `stream`, one launch. A value of
 * `order` outside [0, n_nodes) reads nothing (NaN / -1 rows). Does not synchronise, does not
 * allocate. n_nodes == 0, or no output wanted: returns 0, nothing launched.
 * -2, decided on the host before any device work: a NULL ev or out, negative sizes, more
 * than INT32_MAX / 4 nodes, a missing event array or input column that a wanted output
 * reads (the message names it): order for every output but solo, node_id for node_id,
 * sub_id for solo (which reads nothing else, so solo alone needs neither order nor *in),
 * x, y, z, r for gnn / xyzr, layer_id for layer / vivl.
 * The values of layer_id lie in device memory and are NOT checked, neither on the host nor
 * in the kernel: a negative one gives C's truncating / and %, not the floor division of the
 * NumPy path, so the caller refuses it when it reads the CSV (as DeviceGraph.from_event does). */
int gtf_event_pack(const gtf_event_csr* ev, const gtf_event_cols* in, const gtf_event_out* out, gtf_stream_t stream);

#define GTF_FILL_MAX_COLUMNS 32

/* One column of gtf_fill_columns (an attribute no node or edge of event_conversion.py:53-101
 * holds yet): `rows` rows of row_bytes each at dst, every word of which -- the row itself
 * for 1 and 4 bytes, 8-byte words otherwise -- gets the low bytes of `pattern`. */
typedef struct gtf_fill_column {
    void* dst;           /* device, aligned to the word (1, 4 or 8 bytes); may be NULL with rows == 0 */
    int64_t rows;        /* >= 0 */
    int32_t row_bytes;   /* 1, 4 or a multiple of 8 */
    int32_t pad_;
    uint64_t pattern;    /* e.g. 0x7ff8000000000000 (NaN), 0xffffffff (int32 -1), 0xff (int8 -1), 0, 1 */
} gtf_fill_column;

/* The initial value of every other array of a fresh event (event_conversion.py:53-101 starts
 * from nodes without state dicts; gtf/graph.py empty_arrays, gtf/io.py build_event_csr), the
 * counterpart of gtf_subset_gather's column table: `cols` is a HOST array of at most
 * GTF_FILL_MAX_COLUMNS columns, which travels in the kernel arguments, one launch. One call
 * per axis initialises a gtf_nodes / gtf_states / gtf_edges set: NaN in the float arrays,
 * -1 in uts_rank, uts_side and degree, 0 in has_merged, has_uts and the fresh flags, 1 in
 * has_tse, is_edge, rev_edge and act. Does not synchronise, does not allocate. n_cols == 0,
 * or no column with rows: returns 0, nothing launched.
 * -2, decided on the host before any device work: n_cols outside [0, 32], negative rows, a
 * row_bytes that is neither 1, 4 nor a multiple of 8, a NULL dst with rows > 0, a dst not
 * aligned to its words. */
int gtf_fill_columns(const gtf_fill_column* cols, int32_t n_cols, gtf_stream_t stream);

/* ---- the CSV files themselves: gtf_csv_parse -------------------------------------------
 * The front of event conversion and of the scorer (helper.py:524-543 load_nodes_edges,
 * reconstruction_efficiency.py:41-47: pd.read_csv / np.loadtxt): the bytes of one file in DEVICE
 * memory to selected fields as int64 or double DEVICE columns in row order. gtf_csv.hip.
 *
 * Lines end in "\n" or "\r\n"; the last one may lack it. Blank lines (nothing, or a lone "\r")
 * are skipped and are neither rows nor skipped lines (pandas skip_blank_lines). The first
 * skip_lines non-blank lines are not parsed (1: a header; 2: edges.csv, "<N> <E>" and the
 * header); the caller, who holds the file, resolves header names to field indices. Every row
 * must have exactly n_fields fields of at most GTF_CSV_MAX_ROW_BYTES bytes in all (the line end
 * not counted). Fields that no column asks for are split but not read.
 *
 * A requested field is [+-]digits[.digits][(e|E)[+-]digits] with at least one mantissa digit
 * ("5." and ".5" are numbers) and must lie in the exact domain:
 *   GTF_CSV_INT64   a sign and at most 18 digits, no point, no exponent;
 *   GTF_CSV_DOUBLE  at most 15 mantissa digit characters (leading zeros count, as they do in
 *                   pandas' converter) and a net decimal exponent e = written exponent - digits
 *                   after the point with |e| <= 22; a zero mantissa with any exponent.
 * The value is then M * 10^e (e >= 0) or M / 10^-e: an exact integer, an exact power of ten and
 * ONE correctly rounded fp64 operation, the sign applied by negation ("-0" is -0.0): what
 * pandas.read_csv, np.loadtxt and strtod give, bit for bit. Anything else is not guessed: its
 * GTF_CSV_ERR_* bit is set in counts->error and the first offending (row, field) -- the lowest
 * row, then the lowest field -- is reported with its own bit. */
#define GTF_CSV_MAX_COLUMNS 16
#define GTF_CSV_MAX_FIELDS 64
#define GTF_CSV_MAX_ROW_BYTES 1024
#define GTF_CSV_INT64 0
#define GTF_CSV_DOUBLE 1

#define GTF_CSV_ERR_DIGITS   0x001u  /* more digits than the domain holds */
#define GTF_CSV_ERR_EXPONENT 0x002u  /* |e| > 22 with a nonzero mantissa */
#define GTF_CSV_ERR_TEXT     0x004u  /* nan, inf, text: not the number grammar */
#define GTF_CSV_ERR_EMPTY    0x008u  /* an empty requested field */
#define GTF_CSV_ERR_QUOTE    0x010u  /* a '"' in any field of a row, requested or not */
#define GTF_CSV_ERR_SPACE    0x020u  /* a space or tab inside a requested field */
#define GTF_CSV_ERR_INT_FORM 0x040u  /* a point or an exponent in an int64 column */
#define GTF_CSV_ERR_FIELDS   0x080u  /* not n_fields fields: reported at the first missing or extra field */
#define GTF_CSV_ERR_ROW_LONG 0x100u  /* a row of more than GTF_CSV_MAX_ROW_BYTES bytes: field 0, nothing else of it */
#define GTF_CSV_ERR_ROWS     0x200u  /* more than max_rows rows: row max_rows, field 0 */

typedef struct gtf_csv_column {
    int32_t field;               /* [0, n_fields); no two columns ask for the same field */
    int32_t type;                /* GTF_CSV_INT64 or GTF_CSV_DOUBLE */
    void* out;                   /* [max_rows] int64_t or double, device, 8-byte aligned */
} gtf_csv_column;

typedef struct gtf_csv_in {
    uint32_t struct_size;        /* sizeof(gtf_csv_in) as the caller compiled it */
    uint32_t abi_version;        /* GTF_ABI_VERSION */
    const char* text;            /* [n_bytes] the file, device, 16-byte aligned */
    int32_t n_bytes;             /* < 2^31 - 16 KiB */
    int32_t skip_lines;          /* non-blank lines in front of the rows */
    int32_t n_fields;            /* [1, GTF_CSV_MAX_FIELDS]: every row has exactly this many */
    int32_t max_rows;            /* any upper bound of the row count (newlines + 1): the outputs' size */
    int32_t n_columns;           /* [0, GTF_CSV_MAX_COLUMNS] */
    uint8_t delimiter;           /* ',' ; not a character of the number grammar, '"', a line end or 0 */
    uint8_t pad_[3];
    gtf_csv_column columns[GTF_CSV_MAX_COLUMNS];
} gtf_csv_in;

typedef struct gtf_csv_counts {
    int32_t n_rows;              /* rows parsed (at most max_rows) */
    uint32_t error;              /* GTF_CSV_ERR_* of every offending field */
    int32_t first_bad_row;       /* -1 without an error; rows count from 0 after the skipped lines */
    int32_t first_bad_field;
    uint32_t first_bad_error;    /* the one bit of that field */
    int32_t pad_;
} gtf_csv_counts;

/* The bytes one block takes (4096): a row belongs to the chunk its first byte lies in. */
size_t gtf_csv_chunk_bytes(void);

/* Scratch of gtf_csv_parse: positive for 0 bytes, non-decreasing; about 8 bytes per chunk. */
size_t gtf_csv_parse_workspace_bytes(int32_t n_bytes);

/* Two launches around one hipCUB exclusive sum (line starts per chunk; the rows from LDS), no
 * atomic but the error word's and the first-error key's on a violation, nothing allocated.
 * Synchronises `stream` once, to fill *counts. Nothing is written past out[n_rows] of a column.
 * Returns -2 with counts->error set when a field lies outside the domain (the columns are then
 * unspecified); -3 for another ABI of *in; -2, decided on the host before any launch, for a null
 * argument, negative sizes, a text that is too large or not aligned, n_fields or n_columns out of
 * range, a refused delimiter, a column whose field is out of range or asked for twice, whose type is
 * unknown or whose output is null (max_rows > 0) or unaligned, or a small workspace. n_bytes == 0:
 * returns 0 with zero counts, nothing launched, no workspace needed. */
int gtf_csv_parse(const gtf_csv_in* in, gtf_csv_counts* counts, void* workspace, size_t workspace_bytes,
                  gtf_stream_t stream);

/* ---- a batch's files of one kind in one call: gtf_csv_parse_ev ---------------------------
 * K files with the same field layout lie in ONE device text buffer, file e at files[e].start
 * with files[e].n_bytes bytes. The requested columns come back with the files' rows laid end to
 * end: file e's rows are row_off[e] .. row_off[e + 1] of every column, each exactly what
 * gtf_csv_parse gives on that file alone. The same kernels as gtf_csv_parse (which is the batch
 * of one without tables), one more small launch and one more scan, whatever K is.
 *
 * The table `files` is HOST memory. Every start is a multiple of gtf_csv_chunk_bytes() (so it is
 * 16-byte aligned with the text) and the starts ascend: a file with bytes starts at or behind
 * the end of the one before it, rounded up to a chunk, so every chunk belongs to one file. A
 * file of 0 bytes takes no chunk and may stand anywhere; its start must still be a multiple of
 * the chunk. The last file's end obeys the bound of gtf_csv_in.n_bytes.
 *
 * Bytes outside a file are never read as text: whatever precedes a file's first byte and whatever
 * follows its last one, padding or the next file, reads as '\n'. The padding between files may
 * hold anything.
 *
 * skip_lines holds for every file on its own: rows[e] = max(lines[e] - skip_lines, 0). A file
 * with fewer lines contributes no row and does not shift its neighbours.
 *
 * counts is HOST memory, [n_files]: n_rows, the error bits and the first offending (row, field)
 * of every file, the row counted inside the file after its skipped lines. An error in file e
 * leaves every other file's rows exact; only e's rows are unspecified. max_rows is the size of
 * the columns for the whole batch: the file whose row would be row max_rows of the batch gets
 * GTF_CSV_ERR_ROWS at that row's index inside the file, every later file that has rows gets it
 * at its row 0, and the files in front of it are exact. */
typedef struct gtf_csv_file {
    int32_t start;               /* first byte in the text: a multiple of gtf_csv_chunk_bytes() */
    int32_t n_bytes;
} gtf_csv_file;

typedef struct gtf_csv_in_ev {
    uint32_t struct_size;        /* sizeof(gtf_csv_in_ev) as the caller compiled it */
    uint32_t abi_version;        /* GTF_ABI_VERSION */
    const char* text;            /* the buffer, device, 16-byte aligned */
    const gtf_csv_file* files;   /* [n_files], HOST, starts ascending */
    int32_t* row_off;            /* out, optional: [n_files + 1] device, the files' first rows */
    int32_t n_files;
    int32_t skip_lines;          /* of every file */
    int32_t n_fields;
    int32_t max_rows;            /* the outputs' size: a bound of the batch's rows */
    int32_t n_columns;
    uint8_t delimiter;
    uint8_t pad_[3];
    gtf_csv_column columns[GTF_CSV_MAX_COLUMNS];
} gtf_csv_in_ev;

/* Scratch of gtf_csv_parse_ev for a text whose last file ends at total_bytes: positive for 0,
 * non-decreasing in both; about 8 bytes per chunk and 40 per file. */
size_t gtf_csv_parse_ev_workspace_bytes(int64_t total_bytes, int32_t n_files);

/* The launches of gtf_csv_parse, one launch and one scan over the files between its scan and its
 * parse, one upload of the table; no atomic but a file's error word's and first-error key's on a
 * violation, nothing allocated on the device. Synchronises `stream` once, to fill counts[]. Returns
 * -2 when any file has an error, the message naming the first such file; -3 for another ABI; -2,
 * decided on the host before any launch, for what gtf_csv_parse refuses and for a negative
 * n_files or size, a null table or counts with n_files > 0, a start that is negative, not a
 * multiple of the chunk or in front of the previous file's end. n_files == 0 or no bytes at all:
 * returns 0 with zero counts, row_off (if given) zeroed, no workspace needed. */
int gtf_csv_parse_ev(const gtf_csv_in_ev* in, gtf_csv_counts* counts, void* workspace, size_t workspace_bytes,
                     gtf_stream_t stream);

/* ---- parsed node columns -> the columns of gtf_event_cols: gtf_event_window -------------
 * gtf/io.py read_nodes after the parse (helper.py:524-531): the rows with lo <= layer_id <= hi,
 * both ends inclusive, compacted in file order, and r = sqrt(x*x + y*y) in fp64.
 *
 * r is DEFINED through the C library's pow(x, 2) (helper.py:12-13, gtf/io.py edge_length_xy),
 * which is not always the rounded x * x and differs between C libraries, so it is not ported.
 * Instead the call lists the kept nodes where the two may differ: with p = x * x rounded and
 * e = fma(x, x, -p) the exact residual, a node is AMBIGUOUS when, for its x or its y,
 * | |e| - ulp(p) / 2 | < ulp(p) / 16 -- every pow whose final error is at most 0.5625 ulp agrees
 * with x * x outside that band. amb_index holds their positions among the kept rows, amb_x / amb_y
 * their coordinates. A native caller evaluates sqrt(pow(x, 2) + pow(y, 2)) with its C library for
 * those and writes the results over r with gtf_event_radius_patch; every other r is final. */
typedef struct gtf_window_in {
    uint32_t struct_size;        /* sizeof(gtf_window_in) as the caller compiled it */
    uint32_t abi_version;        /* GTF_ABI_VERSION */
    int32_t n_rows;              /* rows of the node file (gtf_csv_counts.n_rows) */
    int32_t pad_;
    int64_t lo;                  /* min_volume * 1000 */
    int64_t hi;                  /* (max_volume + 1) * 1000 */
    const int64_t* node_idx;     /* [n_rows] */
    const int64_t* layer_id;
    const double* x;
    const double* y;
    const double* z;
} gtf_window_in;

/* Caller-allocated, each [n_rows] (the bound of both counts); none may be NULL with n_rows > 0. */
typedef struct gtf_window_out {
    int64_t* node_idx;
    int64_t* layer_id;
    double* x;
    double* y;
    double* z;
    double* r;
    int32_t* amb_index;
    double* amb_x;
    double* amb_y;
} gtf_window_out;

typedef struct gtf_window_counts {
    int32_t n_kept;
    int32_t n_ambiguous;
} gtf_window_counts;

/* Scratch of gtf_event_window: positive for 0 rows, non-decreasing; about 16 bytes per row. */
size_t gtf_event_window_workspace_bytes(int32_t n_rows);

/* Two launches around one hipCUB exclusive sum of (kept | ambiguous << 32); no atomics, nothing
 * allocated. Synchronises `stream` once, to fill *counts. Nothing is written past [n_kept] of the
 * node columns or [n_ambiguous] of the list. -3 for another ABI of *in; -2 for a null argument or
 * array, a negative or too large n_rows (> INT32_MAX / 4) or a small workspace, decided on the host
 * before any launch. n_rows == 0: returns 0 with zero counts, nothing launched. */
int gtf_event_window(const gtf_window_in* in, const gtf_window_out* out, gtf_window_counts* counts,
                     void* workspace, size_t workspace_bytes, gtf_stream_t stream);

/* gtf_event_window on a batch's rows: row_off is HOST memory, [n_events + 1], from 0 to
 * in->n_rows without decreasing (gtf_csv_parse_ev's offsets); one window for the batch. The kept
 * rows of all events are compacted end to end in batch order, so event e's are the n_kept[e]
 * behind those of the events in front of it; amb_index holds positions among the batch's kept rows
 * and gtf_event_radius_patch takes it as it is. The two launches and the exclusive sum of
 * gtf_event_window and one small gather of the sum at the offsets; one synchronisation, which
 * fills n_kept (HOST, [n_events]) and counts (the batch's totals). workspace:
 * gtf_event_window_ev_workspace_bytes. Refusals as gtf_event_window, and -2 for a negative
 * n_events, null row_off or n_kept with n_events > 0, or offsets that do not start at 0, decrease
 * or do not end at n_rows. */
size_t gtf_event_window_ev_workspace_bytes(int32_t n_rows, int32_t n_events);
int gtf_event_window_ev(const gtf_window_in* in, const int32_t* row_off, int32_t n_events,
                        const gtf_window_out* out, int32_t* n_kept, gtf_window_counts* counts, void* workspace,
                        size_t workspace_bytes, gtf_stream_t stream);

/* r[index[k]] = value[k] for k < n; an index outside [0, n_nodes) writes nothing. One launch, does
 * not synchronise. -2 for negative sizes or a null array with n > 0. */
int gtf_event_radius_patch(double* r, int32_t n_nodes, const int32_t* index, const double* value, int32_t n,
                           gtf_stream_t stream);

/* ---- graph preparation: the optional fields of gtf_graph, built on the GPU -----------
 * The schedules and graph-static slot tables that the lane-group kernels read (every
 * optional field of gtf_graph up to v8 except the packed schedule and the padded tiles),
 * from the base fields alone -- array for array what gtf/device.py builds on the host
 * (node_schedule, sched_segments, sender_schedule, sender_lanes, slot_classes,
 * slot_static_words, slot_sender_xzr). No reference counterpart: the reference walks
 * networkx dicts. gtf_prepare.hip.
 *
 * gtf_graph_tables: device pointers, caller-allocated at the sizes below (N, S, E =
 * n_nodes, n_slots, n_edges); NULL = table not wanted. out_sched and out_lanes are
 * capacities: the first 4 (n_o4 + n_o8 + n_o16) and 2 (4 n_o4 + 8 n_o8) words are written. */
typedef struct gtf_graph_tables {
    int32_t*  slot_dst;       /* [S]   receiver of each slot */
    int32_t*  out_dst;        /* [E]   slot_dst[out_slot] */
    double*   slot_layer;     /* [S]   layer[slot_src], NaN for an orphan key */
    int32_t*  slot_outpos;    /* [S]   position in the sender's out-list, -1 = no edge */
    int32_t*  slot_outidx;    /* [S]   global out-edge index, -1 = no edge */
    uint64_t* slot_class;     /* [S]   written only with slot_sflags and slot_xclass */
    uint8_t*  slot_sflags;    /* [S] */
    uint64_t* slot_xclass;    /* [S] */
    double*   slot_sxzr;      /* [3S]  gnn[slot_src][0, 2, 3], NaN rows for orphan keys */
    uint32_t* slot_static;    /* [S]   needs the three class tables */
    int32_t*  sched;          /* [N] */
    int32_t*  sched_seg;      /* [2N]  needs sched */
    int32_t*  out_sched;      /* [4N] capacity */
    int32_t*  out_lanes;      /* [16N] capacity: 2 * 8 lanes * at most N senders; needs out_sched */
} gtf_graph_tables;

/* Bytes of device scratch gtf_graph_prepare needs (positive for an empty graph too). */
size_t gtf_graph_prepare_workspace_bytes(int32_t n_nodes, int32_t n_slots, int32_t n_edges);

/* Reads only n_nodes, n_slots, n_edges, slot_ptr, slot_src, out_ptr, out_slot, is_edge,
 * rev_edge, gnn and layer of *g; writes every table of *t that was asked for, on `stream`;
 * stores each written table's pointer and the counts n_g2, n_g4, n_g6, n_g8, n_g12, n_g16,
 * n_g32, n_g64, n_big, n_o4, n_o8, n_o16 in *g. The counts come back through one small
 * device-to-host copy: the call SYNCHRONISES `stream` once (after the schedules; the slot
 * and out-edge tables are still in flight on `stream` when it returns, so the workspace
 * stays allocated until `stream` has run them). solo, xyzr,
 * pack_ent / pack_wave, the padded-tile fields and every mutable struct stay the caller's.
 *
 * A table not asked for leaves its optional gtf_graph field NULL (slot_dst and slot_outpos,
 * which gtf_pass requires, are then left as the caller set them), and the dependent fields
 * follow: no sched -> sched_seg NULL and n_g* = n_big = 0; no out_sched -> out_lanes NULL
 * and n_o* = 0; slot_class, slot_sflags and slot_xclass are written and set only when all
 * three were asked for, else all three are NULL (the node kernel reads all three when it
 * sees slot_xclass), and slot_static with them. The orders are the host builders': inside
 * each schedule bucket the narrow sub-class first (<= 2, <= 6, <= 12 slots), ascending
 * node index inside a class; class equality is floating-point == (-0.0 == 0.0; a NaN or an
 * orphan key equals only itself).
 *
 * Status as gtf_pass: -3 for another ABI; -2 for negative sizes, a missing base array or a
 * workspace below gtf_graph_prepare_workspace_bytes, all decided on the host before any
 * launch. n_nodes == 0, or n_slots == n_edges == 0: returns 0 with zero counts and NULL
 * tables, nothing launched (the kernels then take one thread per node). */
int gtf_graph_prepare(gtf_graph* g, const gtf_graph_tables* t, void* workspace, size_t workspace_bytes,
                      gtf_stream_t stream);

/* ---- node removal between two iterations, on the GPU ----------------------------------
 * The packed form of the reference's subGraph.remove_nodes_from(extracted)
 * (extract_track_candidates.py:459-467) followed by dropping the emptied subgraphs: array
 * for array gtf/graph.py's subset() -- kept nodes in order; inside a kept receiver the
 * slots whose sender is kept (an edge or a key of either state dict) in their old order,
 * then the removed senders' surviving dict keys as orphans (slot_src -1, no edge) in the
 * order pack() discovers them: by tse_rank where it is >= 0, then the uts_rank-only keys by
 * uts_rank, ties by old slot index; edge-only slots of removed senders vanish; the out view
 * keeps its successor order; sub_id is renumbered densely. gtf_subset.hip.
 *
 * Three steps, because the sizes of the result are known only after the mask is counted:
 * plan (counts them, SYNCHRONISES once), then the caller allocates, then apply (structure)
 * and gather (payload), neither of which synchronises. Every step reads the plan from the
 * same caller-owned workspace. */
typedef struct gtf_subset_counts {
    int32_t n_nodes, n_slots, n_edges, n_sub;   /* of the result */
} gtf_subset_counts;

/* Device pointers, caller-allocated at the planned sizes (N2, S2, E2 = the counts);
 * NULL = array not wanted. */
typedef struct gtf_subset_out {
    int32_t* node_map;   /* [N2]   old node index of each new node */
    int32_t* slot_map;   /* [S2]   old slot index of each new slot */
    int32_t* slot_ptr;   /* [N2+1] new receiver segments */
    int32_t* slot_src;   /* [S2]   new sender index, -1 for an orphan */
    int32_t* out_ptr;    /* [N2+1] new out view */
    int32_t* out_slot;   /* [E2]   new slot of each surviving out-edge, successor order */
    int32_t* sub_id;     /* [N2]   rank of the old id among the ids that keep a node */
    uint8_t* solo;       /* [N2]   1 = the only kept node of its subgraph */
} gtf_subset_out;

/* How gtf_subset_gather fills the rows of a column (an orphan: new slot_src == -1; the
 * orphan kinds are plain copies on the node axis). */
#define GTF_COL_COPY        0   /* dst row = src row of the old node / slot */
#define GTF_COL_ZERO_ORPHAN 1   /* ... an orphan's row zeroed (is_edge, rev_edge, act) */
#define GTF_COL_NAN_ORPHAN  2   /* ... an orphan's row 8-byte NaNs (edge_mw, send_mw); row_bytes % 8 == 0 */
#define GTF_COL_ZERO_ALL    3   /* every row zeroed, src not read (uts_fresh) */

typedef struct gtf_column {
    const void* src;     /* device: [old rows] of row_bytes each (may be NULL with GTF_COL_ZERO_ALL) */
    void* dst;           /* device: [new rows] of row_bytes each */
    int32_t row_bytes;   /* >= 1 */
    int32_t fill;        /* GTF_COL_* */
} gtf_column;

/* Bytes of device scratch for a subset of a graph of these sizes whose sub_id values lie
 * in [0, n_sub) (extract_track_candidates.py:459-467; gtf/graph.py subset). Positive for an
 * empty graph, non-decreasing in every argument (negative arguments count as 0). */
size_t gtf_graph_subset_workspace_bytes(int32_t n_nodes, int32_t n_slots, int32_t n_edges, int32_t n_sub);

/* Plan (extract_track_candidates.py:459-467; gtf/graph.py subset): reads only n_nodes,
 * n_slots, n_edges, slot_ptr, slot_src, out_ptr, out_slot and is_edge of *g (no optional
 * table), tse_rank / uts_rank [S], sub_id [N] (values in [0, n_sub), any order; a value
 * outside joins no subgraph count) and keep [N] (nonzero = kept), all device arrays.
 * Leaves the old -> new and new -> old node and slot maps, the per-node slot and out-edge
 * offsets and the renumbered sub_id / solo in `workspace`, and the sizes of the result in
 * the host struct *counts, through one small device-to-host copy: the call SYNCHRONISES
 * `stream` once (as gtf_graph_prepare). The workspace is then what gtf_graph_subset_apply
 * and gtf_subset_gather read; it stays the caller's until `stream` has run them.
 * Status: -3 for another ABI; -2 for negative sizes, a missing array (the message names
 * it), slots or edges without nodes, or a workspace below
 * gtf_graph_subset_workspace_bytes, all decided on the host before any launch.
 * n_nodes == 0: returns 0 with zero counts, nothing launched (apply and gather on such a
 * plan must not be called: there is nothing to write). */
int gtf_graph_subset_plan(const gtf_graph* g, const int32_t* tse_rank, const int32_t* uts_rank,
                          const int32_t* sub_id, int32_t n_sub, const uint8_t* keep, void* workspace,
                          size_t workspace_bytes, gtf_subset_counts* counts, gtf_stream_t stream);

/* Apply (extract_track_candidates.py:459-467; gtf/graph.py subset): writes the wanted
 * structure arrays of *out from the plan in `workspace` (*g the graph that was planned).
 * Does not synchronise. Status as the plan (-3 / -2 on the host). */
int gtf_graph_subset_apply(const gtf_graph* g, const void* workspace, const gtf_subset_out* out,
                           gtf_stream_t stream);

/* Payload gather (the row copies of gtf/graph.py subset; extract_track_candidates.py:459-467
 * keeps the attribute dicts of the nodes that stay): for every column, new row i = old row
 * node_map[i] (axis 0) or slot_map[i] (axis 1) of the plan in `workspace`, filled as
 * `fill` says. `cols` is a HOST array; the column table travels in the kernel arguments,
 * many columns per launch. Rows that are multiples of 8 bytes (with 8-byte aligned
 * pointers) move as 8-byte words, of 4 as 4-byte words. Any row_bytes >= 1; a caller's own
 * per-node or per-slot arrays ride along. Does not synchronise. n_cols == 0: returns 0.
 * -2: axis not 0 / 1, row_bytes <= 0, an unknown fill, a NULL dst or (unless
 * GTF_COL_ZERO_ALL) src, GTF_COL_NAN_ORPHAN on rows that are no multiple of 8 bytes. */
int gtf_subset_gather(const void* workspace, int32_t axis, const gtf_column* cols, int32_t n_cols,
                      gtf_stream_t stream);

/* gtf/graph.py refresh_send_mw (the value pack() stores; used after subset(),
 * extract_track_candidates.py:459-467, and by event conversion): for every slot k that is
 * an edge u -> v, send_mw[k] = tse_mw of the slot (receiver u, sender v) when that slot
 * exists and has tse_rank >= 0, else NaN; NaN for every slot that is no edge. Reads
 * n_nodes, n_slots, slot_ptr, slot_src, is_edge (and slot_dst when set) of *g. Relies on the
 * layout invariant that a receiver's non-orphan slots ascend by slot_src (orphans last): a
 * binary search in u's segment. send_mw may not alias tse_mw. Does not synchronise. */
int gtf_refresh_send_mw(const gtf_graph* g, const int32_t* tse_rank, const double* tse_mw, double* send_mw,
                        gtf_stream_t stream);

/* ---- a batch of resident events: gtf_graph_concat / gtf_event_split ---------------------
 * gtf/graph.py concat on the device: K resident graphs in natural layout (what
 * gtf_build_event_csr_device + gtf_event_pack, or gtf_graph_subset_apply, leave) become one
 * graph whose nodes, slots, out-edges and subgraphs are the parts', part after part, with the
 * indices shifted by the sizes of the parts before. Subgraphs of different parts share no
 * edge, so every stage of run_gnn_trackml_mod.sh computes on the fused graph what it computes
 * on each part, and gtf_event_split takes one extraction's outputs apart again. The
 * schedules and slot tables of the fused graph come from gtf_graph_prepare. gtf_concat.hip.
 *
 * The number of launches does not depend on K: one launch for the offsets, one for the
 * structure arrays, one per 32 payload columns. Nothing synchronises, nothing is allocated. */

/* The sizes of one part: a HOST array [n_parts] (the sums are checked before any launch). */
typedef struct gtf_concat_sizes {
    int32_t n_nodes, n_slots, n_edges, n_sub;
} gtf_concat_sizes;

/* One part: an entry of a DEVICE (or host-mapped) array [n_parts]. The sizes repeat the host
 * array's; an array of a part without rows of that kind may be NULL. */
typedef struct gtf_concat_part {
    int32_t n_nodes, n_slots, n_edges, n_sub;
    const int32_t* slot_ptr;   /* [n_nodes+1] */
    const int32_t* slot_src;   /* [n_slots]   -1 = orphan key, kept */
    const int32_t* out_ptr;    /* [n_nodes+1] */
    const int32_t* out_slot;   /* [n_edges] */
    const int32_t* sub_id;     /* [n_nodes]   values in [0, n_sub) */
} gtf_concat_part;

/* The structure arrays of the fused graph, DEVICE arrays at the summed sizes N, S, E;
 * NULL = not wanted. */
typedef struct gtf_concat_out {
    uint32_t struct_size;   /* sizeof(gtf_concat_out) as the caller compiled it */
    uint32_t abi_version;   /* GTF_ABI_VERSION */
    int32_t* slot_ptr;   /* [N+1] */
    int32_t* slot_src;   /* [S] */
    int32_t* out_ptr;    /* [N+1] */
    int32_t* out_slot;   /* [E] */
    int32_t* sub_id;     /* [N] part's sub_id + the subgraphs of the parts before */
    int32_t* event;      /* [N] the part index of every node */
} gtf_concat_out;

#define GTF_CONCAT_MAX_COLUMNS 32

/* One payload column of gtf_concat_columns: dst row (offset of part p + i) = row i of src[p].
 * Rows that are multiples of 8 bytes move as 8-byte words, of 4 as 4-byte words, others as
 * bytes; dst and every src[p] that has rows must be aligned to that word. */
typedef struct gtf_concat_column {
    const void* const* src;   /* DEVICE array [n_parts] of device pointers; an entry of a part without rows is not read */
    void* dst;                /* device: [sum of rows] of row_bytes each */
    int32_t row_bytes;        /* >= 1 */
    int32_t axis;             /* 0 = one row per node, 1 = per slot */
} gtf_concat_column;

/* positive for 0 parts, non-decreasing (a negative count as 0) */
size_t gtf_graph_concat_workspace_bytes(int32_t n_parts);

/* Offsets and structure arrays (gtf/graph.py concat). `sizes` is read on the host, `parts` on
 * the device; the kernels clamp every write to the host sums, so a device table that
 * disagrees with `sizes` writes nothing outside the outputs. Leaves the four offset arrays
 * in `workspace`, which gtf_concat_columns reads: it stays the caller's until `stream` has
 * run those calls. Parts without nodes are legal anywhere. n_parts == 0 or no node at all:
 * slot_ptr[0] = out_ptr[0] = 0 is all that is written.
 * -3: *out built against another layout of this header (struct_size, abi_version).
 * -2, decided on the host before any launch: a NULL sizes, parts, out or workspace, a
 * negative n_parts or size, slots or edges in a part without nodes, a sum of nodes, slots,
 * edges or subgraphs of 2^31 or more, a workspace below gtf_graph_concat_workspace_bytes. */
int gtf_graph_concat(const gtf_concat_sizes* sizes, const gtf_concat_part* parts, int32_t n_parts,
                     const gtf_concat_out* out, void* workspace, size_t workspace_bytes, gtf_stream_t stream);

/* The payload (the np.concatenate of every field in gtf/graph.py concat) after gtf_graph_concat
 * on the same workspace and stream: `cols` is a HOST array of any length, 32 columns travel in
 * the kernel arguments of one launch; only the per-part source pointers lie in device memory.
 * n_nodes / n_slots: the summed sizes given to gtf_graph_concat (the rows of dst per axis).
 * -2: a NULL workspace or column table, negative sizes, row_bytes < 1, an axis that is not
 * 0 / 1, a NULL or misaligned dst, a NULL src table, a column of 2^63 bytes or more. */
int gtf_concat_columns(const void* workspace, int32_t n_parts, int32_t n_nodes, int32_t n_slots,
                       const gtf_concat_column* cols, int32_t n_cols, gtf_stream_t stream);

/* gtf_event_split: the lists of ONE gtf_extract_outputs call on a fused graph, per event.
 * Candidate ids are the smallest node index of their component and candidates ascend by id;
 * the remaining and the fragment groups are in subgraph order; concat and subset keep the node
 * order. So the groups of an event are one run of each list, and the events' runs follow each
 * other in event order: the first group of event e is the lower bound of e among the events
 * of the groups' first members.
 * `in`: the pointer and node-index arrays as gtf_extract_out holds them, with the six host
 * counts of that call; `event` [n_nodes] the fused graph's event column, values in
 * [0, n_events). `out`, DEVICE arrays:
 *   cand_first, rem_first, frag_first [n_events + 1]  the first group of every event (the
 *                                                     last entry: the number of groups)
 *   counts [n_events][6]     gtf_extract_out_counts of every event, in the struct's order
 *   cand_ptr_ev [n_extracted + n_events]  every event's candidate pointers rebased to 0, event
 *                            e's n_e + 1 entries at cand_first[e] + e: with the members from
 *                            in->cand_ptr[cand_first[e]] on, gtf_score_candidates' input
 * The kernels check what the rule relies on: a group without members, a member outside
 * [0, n_nodes), an event outside [0, n_events), members of one group in two events, first
 * members whose events decrease, pointers that decrease or leave the counts. Any of them
 * sets an error word (the only atomic) and the call returns -2 after its one synchronisation;
 * the outputs then hold nothing to rely on, but every write stayed inside them.
 * -3: *in built against another layout of this header (struct_size, abi_version).
 * Also -2, on the host before any launch: a NULL argument or array of a non-empty list,
 * negative sizes, a workspace below gtf_event_split_workspace_bytes. n_events == 0: returns
 * 0, nothing launched. */
typedef struct gtf_split_in {
    uint32_t struct_size;         /* sizeof(gtf_split_in) as the caller compiled it */
    uint32_t abi_version;         /* GTF_ABI_VERSION */
    const int32_t* cand_ptr;      /* [n_extracted + 1] */
    const int32_t* cand_members;  /* [n_extracted_nodes] node indices */
    const int32_t* rem_ptr;       /* [n_remaining + 1] */
    const int32_t* rem_nodes;     /* [n_remaining_nodes] */
    const int32_t* frag_ptr;      /* [n_fragments + 1] */
    const int32_t* frag_nodes;    /* [n_fragment_nodes] */
} gtf_split_in;

typedef struct gtf_split_out {
    int32_t* cand_first;
    int32_t* rem_first;
    int32_t* frag_first;
    int32_t* counts;
    int32_t* cand_ptr_ev;
} gtf_split_out;

size_t gtf_event_split_workspace_bytes(int32_t n_events);
int gtf_event_split(const int32_t* event, int32_t n_nodes, int32_t n_events,
                    const gtf_extract_out_counts* counts, const gtf_split_in* in, const gtf_split_out* out,
                    void* workspace, size_t workspace_bytes, gtf_stream_t stream);

/* ---- Which event of a batch raised: gtf_diag.node_err per event (csrc/gtf_event_errors.hip) ----
 * The error word of a fused graph's workspace says that a reference exception was reproduced,
 * not in which event. With node_err registered (gtf_set_diagnostics) the pass kernels also OR
 * the GTF_ERR_* bits into the raising node's entry; this call reduces that array over the
 * event column that gtf_graph_concat writes and gtf_subset_gather carries, and makes the keep
 * mask that cuts the raising events out (gtf_graph_subset_plan).
 * Inputs, DEVICE arrays:
 *   node_err [n_nodes] uint32   the per-node bits
 *   event    [n_nodes] int32    non-decreasing, values in [0, n_events); NULL: one event
 *                               (n_events must then be 1)
 *   node_id  [n_nodes] int64    or NULL
 *   mask                        the bits that count; the others are ignored
 * Outputs, DEVICE arrays, each may be NULL; the call overwrites every entry of every one given
 * (the caller does not zero them):
 *   err_ev     [n_events] uint32  the OR of the masked bits over the event's nodes
 *   n_raising  [n_events] int32   how many of the event's nodes carry a masked bit
 *   first_node [n_events] int32   the lowest raising node index of the event, in the fused
 *                                 graph's numbering, or -1
 *   first_id   [n_events] int64   node_id[first_node], or -1 for an event without a raising
 *                                 node; written only when node_id is given
 *   keep       [n_nodes]  uint8   1 where the node's event has err_ev == 0
 * host_err_ev, host_n_raising, host_first_node, host_first_id: HOST arrays of the same sizes,
 * each may be NULL, filled from one copy after the call's ONE synchronisation (host_first_id
 * only when node_id is given).
 * Three launches whatever n_events is (initialise, reduce, write out). A node without a masked
 * bit issues no atomic; a raising node issues three on its event's entries. The kernels check
 * what the reduction relies on: event[v] in [0, n_events) and event[v - 1] <= event[v]. A node
 * that breaks either is recorded (the lowest such index, an atomic only on the violation),
 * one whose event is out of range contributes nothing and gets keep 0; the call then returns
 * -2 and gtf_last_error() names that node; the outputs hold nothing to rely on, but every
 * write stayed inside them.
 * Returns 0; -2 also on the host, before any launch: negative sizes, a missing node_err with
 * nodes, event == NULL with n_events != 1, a workspace below
 * gtf_event_errors_workspace_bytes(n_events); -3: *io built against another layout of this
 * header (struct_size, abi_version). n_nodes == 0 or n_events == 0: returns 0, nothing is
 * launched and nothing written. */
typedef struct gtf_event_errors_io {
    uint32_t struct_size;        /* sizeof(gtf_event_errors_io) as the caller compiled it */
    uint32_t abi_version;        /* GTF_ABI_VERSION */
    const uint32_t* node_err;
    const int32_t* event;
    const int64_t* node_id;
    int32_t n_nodes, n_events;
    uint32_t mask;
    uint32_t pad_;
    uint32_t* err_ev;
    int32_t* n_raising;
    int32_t* first_node;
    int64_t* first_id;
    uint8_t* keep;
    uint32_t* host_err_ev;
    int32_t* host_n_raising;
    int32_t* host_first_node;
    int64_t* host_first_id;
} gtf_event_errors_io;

size_t gtf_event_errors_workspace_bytes(int32_t n_events);
int gtf_event_errors(const gtf_event_errors_io* io, void* workspace, size_t workspace_bytes, gtf_stream_t stream);

/* Member order of every extraction candidate as the reference builds it: CCA over the
 * active edges of each subgraph (extract_track_candidates.py:332-346) -- networkx
 * weakly connected components, each copied as subGraph.subgraph(component) (set order
 * when the component is under half the subgraph) -- or the whole subgraph when none of
 * its edges is inactive. order_key[v] = v's position in its candidate: the order
 * rotate_track's stable r-sort and the efficiency's particle vote break ties in.
 * Host arrays of the packed graph; sub_id grouped (pack order). */
typedef struct gtf_candidate_graph {
    int32_t n_nodes, n_slots, n_edges, pad_;
    const int32_t* slot_ptr;
    const int32_t* slot_src;
    const uint8_t* is_edge;
    const uint8_t* act;
    const int32_t* out_ptr;
    const int32_t* out_slot;
    const int32_t* sub_id;
    const int64_t* node_id;
} gtf_candidate_graph;

int gtf_candidate_order(const gtf_candidate_graph* cg, int32_t* order_key);

/* Device memory for a host without a framework allocator (csrc/gtf_mem.hip): the drop-in
 * stage CLIs (extrapolate_merged_states.py:521-572, clustering.py:380-415,
 * remove_state_metadata.py:11-57 -- one process per stage and iteration) allocate and
 * copy through the HIP runtime libgtf is linked against instead of loading a framework
 * (gtf/devmem.py). Copies are stream-ordered; gtf_memcpy_dtoh synchronises the stream.
 * gtf_malloc(…, 0) returns a valid 256-byte allocation (never a null pointer). */
int gtf_device_init(int32_t device);
int gtf_malloc(void** ptr, size_t bytes);
int gtf_free(void* ptr);
int gtf_memcpy_htod(void* dst, const void* src, size_t bytes, gtf_stream_t stream);
int gtf_memcpy_dtoh(void* dst, const void* src, size_t bytes, gtf_stream_t stream);
int gtf_memcpy_dtod(void* dst, const void* src, size_t bytes, gtf_stream_t stream);
int gtf_memset(void* dst, int32_t value, size_t bytes, gtf_stream_t stream);
int gtf_stream_synchronize(gtf_stream_t stream);

const char* gtf_last_error(void);
const char* gtf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GTF_H */
