/*
 * janusgpu.h — C-ABI of libjanusgpu, the MI355X (gfx950) OLAP graph-computer engine
 * behind GpuGraphComputer, the drop-in for JanusGraph's FulgoraGraphComputer.
 *
 * Plain C: pointers + sizes, no torch / HIP / C++ types.  Every entry point returns an int
 * status (JG_OK = 0, < 0 = error class) and never throws or aborts across the ABI; the message
 * of the last failure on the calling thread is available from jg_last_error().
 *
 * What each entry point replaces in the reference (paths relative to
 * /root/reference/janusgraph-core/src/main/java/org/janusgraph/):
 *
 *   jg_ctx_create / jg_ctx_create_rank
 *       FulgoraGraphComputer(StandardJanusGraph, Configuration) + workers(n)
 *       graphdb/olap/computer/FulgoraGraphComputer.java:101-106,134-139
 *   jg_graph_build
 *       the per-superstep edgestore scan: StandardScannerExecutor.run
 *       (diskstorage/keycolumnvalue/scan/StandardScannerExecutor.java:97-216) feeding
 *       VertexJobConverter.process (graphdb/olap/VertexJobConverter.java:122-151: ghost skip)
 *       and the canonical-id map (graphdb/olap/computer/FulgoraVertexMemory.java:74-77).
 *       Done ONCE per computer instead of once per superstep.
 *   jg_graph_build_edgestore
 *       the same, from the raw rows: the row decode of VertexJobConverter.process and
 *       EdgeSerializer.parseRelation (graphdb/database/EdgeSerializer.java:86-122) on the GPU
 *   jg_builder_keep_labels / jg_builder_finish_labels
 *       the typed vertex-centric queries of a MessageScope.Local such as __.inE("battled")
 *       (graphdb/olap/computer/VertexProgramScanJob.java:126-134,
 *       graphdb/query/vertex/BasicVertexCentricQueryBuilder.java:482-587)
 *   jg_pagerank (+ begin/step/end)
 *       executeVertexProgram superstep loop (FulgoraGraphComputer.java:210-230) running
 *       janusgraph-backend-testutils/.../olap/PageRankVertexProgram.java:89-110, with the gather of
 *       VertexMemoryHandler.receiveMessages (graphdb/olap/computer/VertexMemoryHandler.java:121-151)
 *   jg_shortest_distance
 *       the same loop running ShortestDistanceVertexProgram.java:112-146 with
 *       ShortestDistanceMessageCombiner.java:29-31 (min)
 *   jg_bfs
 *       TinkerPop ShortestPathVertexProgram under Fulgora's forced {Local(bothE), Global} scopes
 *       (FulgoraGraphComputer.java:249-253): hop depth per source (paths are rebuilt host-side)
 *   jg_connected_components
 *       TinkerPop ConnectedComponentVertexProgram (String-min label over BOTH edges,
 *       VertexProgramScanJob.java:113-135 loads BOTH); pinned by OLAPTest.java:736-762
 *   jg_peer_pressure
 *       TinkerPop PeerPressureVertexProgram (weighted mode of the neighbours' cluster votes over outE or
 *       bothE, optional vote distribution), under the same loop; ties go to the smallest cluster id
 *   jg_sssp_keep / jg_sssp_kept_dag
 *       TinkerPop ShortestPathVertexProgram with distanceProperty(key) and edgeDirection(dir) [TP-recall]:
 *       summed edge weights along the direction's edges, and the minimum-weight paths' predecessor DAG
 *   jg_graph_set_weights_f64 / jg_sssp_keep_f64 / jg_sssp_kept_dag_f64
 *       the same program over a Double distanceProperty: IEEE binary64 sums, exact ties only
 *   JG_ADJ_EDGE_INDEX / jg_bfs_kept_dag_edges / jg_sssp_kept_dag_edges
 *       the same program with includeEdges(true) [TP-recall]: a path is v, e, v, ..., v, so the snapshot numbers
 *       its edges and the DAGs list one entry per edge, parallel edges apart
 *   jg_combine_steps
 *       the same loop for sum/min/max MessageCombiner programs (OLAPTest.DegreeCounter,
 *       janusgraph-test/.../olap/OLAPTest.java:424-503; VertexState.java:85-114)
 *   jg_graph_info_get / jg_ctx_last_stats
 *       ScanMetrics counters (StandardScanMetrics.java:28-88: ghost-vertices, truncated-results)
 *       and memory().getIteration()/getRuntime() (FulgoraMemory.java:97-101)
 *
 * Ownership: host arrays passed in are caller-owned and read only during the call; outputs are
 * caller-allocated.  Device memory is owned by the library (per jg_graph) and handed back to the
 * device by jg_graph_destroy (the library's block cache, which spares a build its ~250 device
 * synchronising frees, is emptied there and by jg_ctx_trim).  A jg_ctx is not re-entrant: one call in
 * flight per context, and a jg_graph belongs to its context's caller thread (read-only queries such as
 * jg_graph_neighbors may run from several threads: their lazily made host copies are locked).
 */
#ifndef JANUSGPU_H
#define JANUSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: jg_graph_info.exchange_values appended; jg_bfs_rows, jg_graph_neighbors added.
 * 3: jg_bfs_keep, jg_bfs_kept_row, jg_bfs_kept_release, jg_ctx_trim added.  Callers must check
 * jg_abi_version() == JG_ABI_VERSION before passing any struct across the ABI.
 * Still 3 (entry points only, no layout change): jg_builder_keep_labels, jg_builder_add_labeled_edges,
 * jg_builder_finish_labels added; jg_bfs_kept_dag, jg_bfs_kept_dag_read added; jg_cc_census, jg_cc_census_read,
 * jg_cc_census_release added; jg_pagerank_top, jg_pagerank_top_read, jg_pagerank_top_release added;
 * jg_peer_pressure added; JG_ADJ_WEIGHT_BOTH, jg_sssp_keep, jg_sssp_kept_row, jg_sssp_kept_release,
 * jg_sssp_kept_dag, jg_sssp_kept_dag_read added; JG_ADJ_EDGE_INDEX, jg_graph_neighbor_edges,
 * jg_bfs_kept_dag_edges, jg_bfs_kept_dag_read_edges, jg_sssp_kept_dag_edges, jg_sssp_kept_dag_read_edges added;
 * jg_graph_set_weights_f64, jg_sssp_keep_f64, jg_sssp_kept_row_f64, jg_sssp_kept_dag_f64,
 * jg_sssp_kept_dag_edges_f64, jg_sssp_kept_dag_read_f64 added; jg_builder_keep_relations,
 * jg_builder_set_weight_key_f64, jg_graph_edge_relations, jg_bfs_kept_dag_read_relations,
 * jg_sssp_kept_dag_read_relations added; jg_builder_keep_scope_ordinals, jg_graph_scope_positions added. */
#define JG_ABI_VERSION 3

/* ---- status codes ---- */
#define JG_OK               0
#define JG_ERR_ARG         -1  /* bad argument (null pointer, size, unknown vertex id …)        */
#define JG_ERR_OOM         -2  /* device or host allocation failed                                */
#define JG_ERR_HIP         -3  /* HIP runtime error                                               */
#define JG_ERR_RCCL        -4  /* RCCL communicator / collective error                            */
#define JG_ERR_UNSUPPORTED -5  /* operation not available for this graph/context configuration  */
#define JG_ERR_STATE       -6  /* call out of order (e.g. step before begin)                      */

/* ---- adjacency requested at build time (bit flags) ---- */
#define JG_ADJ_OUT  1u  /* out-adjacency: rows = source vertex (bottom-up of IN traversals)        */
#define JG_ADJ_IN   2u  /* in-adjacency:  rows = target vertex (PageRank pull, SD push)           */
#define JG_ADJ_BOTH 4u  /* symmetrised:   rows = every vertex, a self-loop appears twice (BOTH)   */
/* With JG_ADJ_BOTH and edge weights only (a weight array, or a builder whose chunks carry weights; anything
 * else is JG_ERR_ARG): the BOTH adjacency carries each edge's weight on both of its entries (jg_sssp_keep
 * with JG_DIR_BOTH relaxes it).  Without the flag a build is what it was before the flag existed. */
#define JG_ADJ_WEIGHT_BOTH 8u
/* Every adjacency the build makes keeps a uint32 edge ordinal beside each entry: the position of the entry's
 * edge in the caller's edge list (jg_graph_build: the index into src/dst[0, m); a builder fed ids: the position
 * in the concatenation of its jg_builder_add_edges / jg_builder_add_labeled_edges chunks, in call order).
 * Ghost edges and self-loops keep their positions: ordinals count what the caller gave, not what survived.  On
 * BOTH both entries of an edge carry its ordinal (a self-loop: two entries of one row).  Inside a run of equal
 * neighbours of a row, ordinals ascend.  Read back by jg_graph_neighbor_edges and listed by the edge-listing
 * predecessor DAGs (jg_bfs_kept_dag_edges, jg_sssp_kept_dag_edges).
 * A jg_builder_add_rows builder that opted in (jg_builder_keep_relations or jg_builder_set_weight_key_f64) numbers
 * the decoder's kept list instead: every visible OUT user edge of a kept row, in chunk order then entry order,
 * ghost-ended edges included.
 * JG_ERR_UNSUPPORTED with the flag: graphs of several shards (logical shards, rank mode); jg_builder_add_rows
 * builders without such an opt-in and jg_graph_build_edgestore (the relation ids the decoder computes are not kept);
 * jg_builder_finish_labels on a builder without jg_builder_keep_scope_ordinals (its select compacts the list; with
 * the opt-in the scope's kept list is the edge list); jg_graph_build_rmat (no caller edge list).
 * Without the flag a build is what it was before the flag existed: no allocation, no sort payload, no launch. */
#define JG_ADJ_EDGE_INDEX 16u

/* ---- traversal direction (the MessageScope.Local incident traversal) ---- */
#define JG_DIR_OUT  1   /* follow u->v edges from u          */
#define JG_DIR_IN   2   /* follow u->v edges from v back to u */
#define JG_DIR_BOTH 3

/* Fulgora's hard limit on entries per non-BOTH slice (graphdb/olap/QueryContainer.java:42,133) */
#define JG_FULGORA_HARD_QUERY_LIMIT 100000

typedef struct jg_ctx jg_ctx;
typedef struct jg_graph jg_graph;

typedef struct jg_graph_info {
    int64_t num_vertices;        /* |V| handed to the build (existing, non-ghost vertices)          */
    int64_t num_edges;           /* edges kept: both endpoints in V                                  */
    int64_t ghost_edges;         /* edges dropped because an endpoint is not in V                    */
    int64_t self_loops;          /* kept edges with src == dst                                       */
    int64_t truncated_vertices;  /* without a query limit: vertices with > JG_FULGORA_HARD_QUERY_LIMIT
                                    edge entries (in+out), whose OUT/IN slices Fulgora truncates and
                                    this graph does not.  Built with jg_builder_set_query_limit: the
                                    rows whose edge slice reached the limit (Fulgora's
                                    truncated-results metric, VertexJobConverter.java:139)          */
    int64_t max_in_degree;
    int64_t max_out_degree;
    int64_t device_bytes;        /* device memory held by this graph, summed over shards             */
    int32_t num_shards;          /* 1D vertex partitions (one per device / rank)                    */
    uint32_t flags;              /* JG_ADJ_* actually built                                          */
    int64_t exchange_values;     /* vertex values this process's shards receive from peers per
                                    exchange step of the pull vector (IN adjacency if built, else
                                    BOTH): the sparse halo, or (P-1)*S each for the dense allgather;
                                    0 on one shard                                                   */
} jg_graph_info;

typedef struct jg_stats {
    int32_t supersteps;          /* memory().getIteration() of the equivalent Fulgora run           */
    int32_t levels;              /* passes actually executed on the GPU; the unit depends on the path:
                                  * BFS: levels; CC: union-find BFS levels or propagation sweeps;
                                  * shortest distance: supersteps (hop-bounded Bellman-Ford) or, on the
                                  * unbounded delta-stepping path, near-far passes      */
    double  build_ms;            /* last jg_graph_build*: snapshot -> CSR on device                 */
    double  compute_ms;          /* last program: HIP-event time of the superstep loop              */
    double  exchange_ms;         /* HIP-event time of the exchange steps (profiling on, sharded)    */
    double  kernel_ms_total;     /* sum of HIP-event durations of the dominant kernel                */
    int64_t kernel_launches;     /* number of launches of the dominant kernel that were timed       */
    double  algorithmic_bytes;   /* SURVEY §8(d) byte model for the last program, whole run         */
    double  edges_traversed;     /* adjacency entries examined (for TEPS)                           */
} jg_stats;

/* ---- library / context ---- */
int         jg_abi_version(void);
const char* jg_last_error(void);

/* One process driving `ndev` devices (the JVM case).  ndev > 1 shards the graph 1D over the listed
 * devices; distinct devices exchange through RCCL (ncclCommInitAll), a device listed more than once
 * holds several logical shards that exchange by device copies (test mode). */
int jg_ctx_create(const int* devices, int ndev, jg_ctx** out);

/* One process per GPU (torch.distributed style): this process is `rank` of `nranks`, driving
 * `device`.  `unique_id` is the JG_UNIQUE_ID_BYTES blob from jg_comm_unique_id() on rank 0,
 * broadcast out-of-band by the caller.  nranks == 1 needs no unique_id (may be NULL). */
#define JG_UNIQUE_ID_BYTES 128
int jg_comm_unique_id(void* out /* JG_UNIQUE_ID_BYTES */);
int jg_ctx_create_rank(int device, int nranks, int rank, const void* unique_id, jg_ctx** out);
/* The same rank mode over a caller-supplied host transport instead of RCCL: every exchange step is
 * staged through host memory and handed to these callbacks (synchronous, called by every rank in
 * the same order).  For tests of the multi-process control flow where RCCL cannot run (two ranks
 * on one GPU); the same code paths build, plan, pack and place the data as with RCCL.
 *   allgather: out[r * bytes .. (r + 1) * bytes) = rank r's `in`, for every rank r.
 *   exchange:  send[i] (send_bytes[i] bytes) to rank send_peer[i]; receive recv_bytes[i] bytes from
 *              rank recv_peer[i] into recv[i].  Zero-byte transfers are not listed.
 * Callbacks return 0 on success.  `t` is copied; `t->user` is passed back untouched. */
typedef struct jg_transport {
    void* user;
    int (*allgather)(void* user, const void* in, void* out, size_t bytes);
    int (*exchange)(void* user, int nsend, const int* send_peer, const void* const* send, const size_t* send_bytes,
                    int nrecv, const int* recv_peer, void* const* recv, const size_t* recv_bytes);
} jg_transport;
int jg_ctx_create_rank_transport(int device, int nranks, int rank, const jg_transport* t, jg_ctx** out);
/* Lifetime: every jg_graph and jg_builder made from a context uses its streams and communicators, so
 * destroy them before the context.  While any is alive jg_ctx_destroy changes nothing and returns
 * JG_ERR_STATE (the context stays valid: destroy the graphs/builders, then call it again). */
int jg_ctx_destroy(jg_ctx* ctx);
/* Hands the device memory the library caches for reuse (freed blocks) back to the context's devices. */
int jg_ctx_trim(jg_ctx* ctx);
int jg_ctx_last_stats(const jg_ctx* ctx, jg_stats* out);
/* Record HIP events around every launch of the dominant kernel (costs ~1 us per launch). */
int jg_ctx_set_profiling(jg_ctx* ctx, int enable);

/* ---- graph snapshot ---- */
/* vid[n]: the ids of the vertices the scan returned (unique, any order; outputs are indexed the same
 * way).  src/dst[m]: edge endpoints as vertex ids; an edge whose endpoint is not in vid is a ghost
 * edge and is dropped.  weight[m] (nullable): Integer edge property for jg_shortest_distance; NULL
 * means unit weights.  Multi-edges and self-loops are kept (JanusGraph MULTI semantics). */
int jg_graph_build(jg_ctx* ctx, const int64_t* vid, int64_t n,
                   const int64_t* src, const int64_t* dst, const int32_t* weight, int64_t m,
                   uint32_t flags, jg_graph** out);

/* The same snapshot straight from the edgestore rows the scan returns, decoded on the GPU
 * (replaces VertexJobConverter.process + EdgeSerializer.parseRelation per row and entry:
 * graphdb/olap/VertexJobConverter.java:122-151,169-181; graphdb/database/EdgeSerializer.java:86-122;
 * graphdb/idmanagement/IDManager.java:496-506).  Row r has key row_keys[r] (the 8-byte big-endian
 * StaticBuffer as an unsigned value) and entries [row_entry_off[r], row_entry_off[r+1]); entry e is
 * bytes[entry_off[e] .. entry_off[e+1]) with its value at value_pos[e] (as jg_decode_edges; the
 * type table gives edge-label multiplicities).  Rows with an odd key (schema / invisible vertices)
 * are filtered; a row whose first entry is not the VertexExists property is a ghost; the kept rows
 * are V (in row order, ids -> vid_out[nrows], count -> *num_vertices_out, both nullable) and their
 * OUT entries of visible user edges are the edges (ghost endpoints dropped as in jg_graph_build).
 * Unit weights.  Partitioned (vertex-cut) vertices are one vertex, the canonical id
 * (IDManager.java:525-551): every representative row adds its edges, only the canonical row's
 * VertexExists decides the ghost rule (VertexProgramScanJob.java:88-102).  A malformed entry on a
 * kept row or a key with no user vertex type: JG_ERR_ARG.  Stats: build_ms (whole snapshot),
 * exchange_ms (the row copies), kernel_ms_total (copies + decode kernels). */
int jg_graph_build_edgestore(jg_ctx* ctx, const uint64_t* row_keys, int64_t nrows, const int64_t* row_entry_off,
                             const uint8_t* bytes, int64_t nbytes, const int64_t* entry_off, const int32_t* value_pos,
                             int64_t nentries, const int64_t* type_ids, const int8_t* type_mult, int32_t ntypes,
                             int32_t partition_bits, uint32_t flags, int64_t* vid_out, int64_t* num_vertices_out,
                             jg_graph** out);

/* ---- chunked snapshot ----
 * The same two snapshots fed in chunks as the scan produces them (Java direct ByteBuffers hold at most
 * 2 GiB, and the scan is a stream: StandardScannerExecutor.java:141-174 hands rows to the processors
 * in key order).  Either ids (add_vertices / add_edges, any interleaving; edge weights on every
 * add_edges call or on none) or raw rows (set_schema once, then add_rows; a row never spans two
 * chunks), not both.  Each add_rows call stages its chunk and returns while the chunk is copied and
 * decoded on the GPU, so the decode overlaps the caller's scan of the next chunk.  finish builds the
 * graph exactly as jg_graph_build / jg_graph_build_edgestore would from the concatenated chunks
 * (vertex order = the order added; read it back with jg_graph_vertex_ids).  The builder is single-use;
 * destroy it after finish (or instead of it).  Stats of finish: build_ms, kernel_ms_total = copy +
 * decode time of the rows (HIP events per chunk, summed), exchange_ms = their host -> device copies
 * alone, kernel_launches = number of row chunks.  Chunks whose entries are all shorter than 256 bytes
 * cross PCIe with 1-byte lengths and value positions instead of the int64 offsets and int32 positions. */
typedef struct jg_builder jg_builder;
int jg_builder_create(jg_ctx* ctx, jg_builder** out);
int jg_builder_add_vertices(jg_builder* b, const int64_t* vid, int64_t n);
int jg_builder_add_edges(jg_builder* b, const int64_t* src, const int64_t* dst, const int32_t* weight, int64_t m);
int jg_builder_set_schema(jg_builder* b, const int64_t* type_ids, const int8_t* type_mult, int32_t ntypes,
                          int32_t partition_bits);
/* entry_weight[nentries] (nullable; on every chunk or none): the Integer weight property of each
 * entry's edge for jg_shortest_distance (JG_WEIGHT_ABSENT: the edge has none), read by the caller
 * with the edge's own serializer; ignored for entries that are not kept edges. */
int jg_builder_add_rows(jg_builder* b, const uint64_t* row_keys, int64_t nrows, const int64_t* row_entry_off,
                        const uint8_t* bytes, int64_t nbytes, const int64_t* entry_off, const int32_t* value_pos,
                        const int32_t* entry_weight, int64_t nentries);
/* Fulgora's per-row slice cap (graphdb/olap/QueryContainer.java:42,121-146): an untyped OUT or IN edge
 * scope is not a fitted query (query/vertex/BasicVertexCentricQueryBuilder.java:451-456), so the scan
 * loads each row's EDGE slice (IDHandler.getBounds(EDGE), idhandling/IDHandler.java:172-193: the visible
 * user edges of both directions, contiguous in column order) with at most `limit` entries
 * (inmemory/SinglePageEntryBuffer.java:54-77 stops there), and a program reads only the entries of its
 * direction among them.  With limit > 0 (JG_FULGORA_HARD_QUERY_LIMIT reproduces Fulgora) the graph is
 * built from what the programs would read: the OUT adjacency and out-degrees (PageRank's edgeCount)
 * from the OUT entries within their row's first `limit`; the IN adjacency, for in_entries = JG_DIR_IN,
 * from the IN entries within their row's first `limit` (PageRank's gather and a combiner over IN:
 * receivers read their own IN entries) or, for JG_DIR_OUT, as the transpose of the capped OUT entries
 * (ShortestDistance: a receiver reads its OUT entries, the IN adjacency is pushed along); BOTH is a
 * fitted query and never capped.  limit = 0 (the default) builds the untruncated graph.  Rows only
 * (jg_builder_add_rows); call before the first chunk. */
int jg_builder_set_query_limit(jg_builder* b, int64_t limit, int32_t in_entries);
/* Edge weights decoded on the GPU from the rows (ShortestDistanceVertexProgram's Integer property,
 * ShortestDistanceVertexProgram.java:69) instead of per-entry host weights: an edge's properties follow
 * its ids in its value as (inline key id, value) pairs in ascending key-id order
 * (graphdb/database/EdgeSerializer.java:294-302; inline id = IDManager.stripRelationTypePadding(key id),
 * VariableLong.writePositive, idhandling/IDHandler.java:155-158; values per StandardSerializer.writeObject:
 * a null flag byte unless String, then the attribute serializer's bytes).  weight_key = the inline id of the
 * weight key; key_ids / key_types (nkeys) = every property key an edge may carry before it, with its
 * JG_PROP_* type (an edge holding a key of unknown type before the weight: JG_ERR_UNSUPPORTED at finish).
 * The weight is JG_WEIGHT_ABSENT where the edge has no non-null Integer value for the key; a stored
 * Integer.MIN_VALUE collides with that marker and fails the build (JG_ERR_UNSUPPORTED).  The edge labels
 * must have no signature keys (their values precede the inline pairs without ids): the caller checks.
 * Rows only, before the first chunk; add_rows then takes no entry_weight. */
#define JG_PROP_BYTE   1
#define JG_PROP_SHORT  2
#define JG_PROP_INT    3
#define JG_PROP_LONG   4
#define JG_PROP_CHAR   5
#define JG_PROP_BOOL   6
#define JG_PROP_DATE   7
#define JG_PROP_FLOAT  8
#define JG_PROP_DOUBLE 9
#define JG_PROP_UUID   10
#define JG_PROP_STRING 11
int jg_builder_set_weight_key(jg_builder* b, int64_t weight_key, const int64_t* key_ids, const int8_t* key_types,
                              int32_t nkeys);
/* ---- edge identity and fp64 weights from rows ----
 * Both are opt-in: a rows builder that calls neither behaves as before (JG_ADJ_EDGE_INDEX: JG_ERR_UNSUPPORTED).
 *
 * jg_builder_keep_relations: the decoder keeps each kept edge's JanusGraph relation id (the id
 * EdgeSerializer.parseRelation reads beside the other vertex; what the Java side detaches an Edge by) aligned
 * with the edge list.  Must precede every chunk (else JG_ERR_STATE); rows only (jg_builder_add_vertices /
 * _add_edges / _add_labeled_edges on such a builder: JG_ERR_ARG); mutually exclusive with a positive
 * jg_builder_set_query_limit, in either order (the second of the two: JG_ERR_STATE); may be combined with
 * jg_builder_keep_labels (jg_builder_finish_labels keeps refusing JG_ADJ_EDGE_INDEX unless the builder also
 * called jg_builder_keep_scope_ordinals; then the scope's compacted relation table moves into the scoped graph).
 * jg_builder_finish(flags | JG_ADJ_EDGE_INDEX) then succeeds on one shard (several shards, rank mode:
 * JG_ERR_UNSUPPORTED).  The graph's edge list is the decoder's kept list (see JG_ADJ_EDGE_INDEX), ordinals index
 * it, and the relation table (8 B per listed edge, counted in jg_graph_info.device_bytes) moves into the graph.
 * Finished without the flag, the table is dropped and the graph is the plain one.
 *
 * jg_graph_edge_relations: rel_out[i] = the relation id of edge ordinal ordinals[i], gathered on the device.
 * A graph without the table (built from ids, or without the opt-in and the flag): JG_ERR_UNSUPPORTED; an ordinal
 * >= the list length: JG_ERR_ARG (checked on the device; nothing out of range is read); count == 0: JG_OK.
 * jg_bfs_kept_dag_read_relations / jg_sssp_kept_dag_read_relations (the latter for the integer and the f64
 * edge-listing DAG): the relation ids of entries [off[first], off[first + count]) of the held edge-listing DAG,
 * parallel to pred_out: one device gather through the held ordinals, one copy out.  Errors as for the
 * _read_edges pair, plus JG_ERR_UNSUPPORTED without the table.
 *
 * jg_builder_set_weight_key_f64: arguments and call rules of jg_builder_set_weight_key; setting both weight keys
 * on one builder is JG_ERR_STATE.  The weight key's type decides how its value is read, one double per edge:
 *   JG_PROP_DOUBLE  8 bytes, the big-endian IEEE bits (DoubleSerializer.write);
 *   JG_PROP_LONG    8 bytes, big-endian value - Long.MIN_VALUE (LongSerializer), converted exactly;
 *   JG_PROP_INT     a signed VariableLong, converted exactly;
 *   JG_PROP_FLOAT (TinkerPop adds Floats in binary32), any other type, or a key absent from the table:
 *   JG_ERR_UNSUPPORTED from this call.
 * An integer value with |v| > 2^53 fails its chunk's completion with JG_ERR_UNSUPPORTED; a value cut short by its
 * entry's end is a malformed entry (JG_ERR_ARG).  An edge without the property or with a null value gets NaN.
 * The builder must be finished with JG_ADJ_EDGE_INDEX (without: JG_ERR_ARG), which this call permits on its own;
 * the finish then does what jg_graph_set_weights_f64 does on the same values (statistics, gate, automatic delta
 * and error codes: a NaN, zero, negative or infinite weight anywhere in the list JG_ERR_ARG, an absorbing range
 * JG_ERR_UNSUPPORTED).  A failed finish builds no graph and leaves the builder destroyable.  Afterwards
 * jg_sssp_keep_f64 and the _f64 DAG calls work as on an ids graph, and a later jg_graph_set_weights_f64 (m = the
 * list length) replaces the weights.  JG_ADJ_WEIGHT_BOTH is not needed and its rule is unchanged. */
int jg_builder_keep_relations(jg_builder* b);
int jg_builder_set_weight_key_f64(jg_builder* b, int64_t weight_key, const int64_t* key_ids, const int8_t* key_types,
                                  int32_t nkeys);
int jg_graph_edge_relations(const jg_graph* g, const uint32_t* ordinals, int64_t count, int64_t* rel_out);
int jg_bfs_kept_dag_read_relations(jg_graph* g, int64_t first, int64_t count, int64_t* rel_out);
int jg_sssp_kept_dag_read_relations(jg_graph* g, int64_t first, int64_t count, int64_t* rel_out);
int jg_builder_finish(jg_builder* b, uint32_t flags, jg_graph** out);
/* ---- label-scoped graphs (typed message scopes) ----
 * Fulgora turns each MessageScope.Local of a program into a vertex-centric query
 * (graphdb/olap/computer/VertexProgramScanJob.java:126-134); a scope written __.inE("battled") becomes a
 * typed query with one slice per label (graphdb/query/vertex/BasicVertexCentricQueryBuilder.java:482-587).
 * Those slices are fitted, so the 100000-entry cap of graphdb/olap/QueryContainer.java:133 never applies to
 * them.  Here one snapshot yields any number of label-scoped graphs: the builder keeps a label beside
 * every edge, and jg_builder_finish_labels cuts a scope out of the accumulated edge list on the GPU.
 *
 * jg_builder_keep_labels: must precede every chunk (a builder that holds a chunk or is finished:
 * JG_ERR_STATE).  Mutually exclusive with a positive jg_builder_set_query_limit, in either order: the
 * second of the two returns JG_ERR_STATE (typed scopes are fitted, never capped).
 *   Rows (jg_builder_add_rows, unchanged otherwise): the label of a kept edge is its relation type id, the
 *   value jg_decode_edges returns in type_out.
 *   Ids: every edge chunk arrives through jg_builder_add_labeled_edges, label[m] opaque int64 values (weights
 *   on every chunk or none, as jg_builder_add_edges); plain jg_builder_add_edges on a label-keeping builder
 *   returns JG_ERR_ARG, jg_builder_add_labeled_edges without jg_builder_keep_labels JG_ERR_STATE.
 *
 * jg_builder_finish_labels: the graph of ALL vertices added (V is never filtered) and of the edges whose
 * label is in labels[0, nlabels).  Duplicates in labels are ignored; a label no edge carries matches
 * nothing (BasicVertexCentricQueryBuilder.java:484 skips unknown types) and legally gives zero edges.
 * nlabels < 1, null labels or more than JG_MAX_SCOPE_LABELS distinct labels: JG_ERR_ARG; without
 * jg_builder_keep_labels: JG_ERR_STATE.  The call completes the pending chunks and seals the builder (later
 * add_* calls: JG_ERR_STATE) but does not finish it: it may be called any number of times, and a final
 * jg_builder_finish is still allowed (it covers every label, then finishes the builder as always).  Every
 * graph of one builder reports the same jg_graph_vertex_ids and survives jg_builder_destroy.  The
 * jg_graph_info counts (num_edges, ghost_edges, self_loops, max degrees) describe the scope only, and the
 * 2^32-1 edge limit applies to the scope, not to the accumulated list.  flags, logical shards and rank mode
 * behave as in jg_builder_finish.  Stats: build_ms (the whole call), kernel_ms_total = HIP-event time of
 * the scope select, kernel_launches = the select's own launches (the count, then the scatter if anything is
 * kept; 0 for an empty edge list), algorithmic_bytes = 16 B per accumulated edge (its label read twice) +
 * 2 x 16 B (20 B with weights) per kept edge (read, then written).
 *
 * Edge ordinals in a scope.  jg_builder_finish_labels(flags | JG_ADJ_EDGE_INDEX) is JG_ERR_UNSUPPORTED (the select
 * compacts the edge list) unless the builder opted in:
 * jg_builder_keep_scope_ordinals: must precede every chunk (else JG_ERR_STATE); needs jg_builder_keep_labels, in
 * either order (checked at jg_builder_finish_labels: JG_ERR_STATE).  A builder that never calls it behaves as before.
 * With it, jg_builder_finish_labels(flags | JG_ADJ_EDGE_INDEX) succeeds on one shard (several shards, rank mode:
 * JG_ERR_UNSUPPORTED).  The scoped graph's edge list is the scope's kept list: ordinal k is the k-th kept edge in
 * accumulated order (the select is a stable compaction), so jg_graph_neighbor_edges, both _kept_dag_edges families
 * and jg_graph_set_weights_f64 (m = the kept count) behave as on a graph jg_builder_finish built from those edges
 * alone.  The same scatter pass carries along, per kept edge: its position in the accumulated list (8 B, written
 * only; the table moves into the graph, counted in jg_graph_info.device_bytes); on a rows builder with
 * jg_builder_keep_relations its relation id (the compacted table moves into the graph: jg_graph_edge_relations and
 * the _kept_dag_read_relations calls work; the builder's own table stays for later scopes and a final
 * jg_builder_finish); on a rows builder with jg_builder_set_weight_key_f64 its decoded double, and the finish then
 * does what jg_graph_set_weights_f64 does on the scope's doubles only (a NaN on an edge outside the scope is legal; a
 * bad value inside it: the same error codes, no graph, the builder stays usable).  Without the flag the opt-in
 * changes nothing.  Stats: algorithmic_bytes grows by 8 B per kept edge for the positions and by 16 B per kept edge
 * for each of the other two columns; kernel_launches is unchanged.
 * jg_graph_scope_positions: pos_out[i] = the accumulated-list position of ordinal first + i, for [first, first +
 * count).  A graph without the table: JG_ERR_UNSUPPORTED; a range outside the list: JG_ERR_ARG; count == 0: JG_OK. */
#define JG_MAX_SCOPE_LABELS 1024
int jg_builder_keep_labels(jg_builder* b);
int jg_builder_keep_scope_ordinals(jg_builder* b);
int jg_graph_scope_positions(const jg_graph* g, int64_t first, int64_t count, int64_t* pos_out);
int jg_builder_add_labeled_edges(jg_builder* b, const int64_t* src, const int64_t* dst, const int32_t* weight,
                                 const int64_t* label, int64_t m);
int jg_builder_finish_labels(jg_builder* b, const int64_t* labels, int32_t nlabels, uint32_t flags, jg_graph** out);
int jg_builder_destroy(jg_builder* b);
/* vid_out[i] = the id of vertex offset + i in output order (the order vid[] / the kept rows were given). */
int jg_graph_vertex_ids(const jg_graph* g, int64_t offset, int64_t count, int64_t* vid_out);

/* Synthetic Graph500 Kronecker (RMAT a,b,c,d = .57,.19,.19,.05) graph generated on the device(s):
 * n = 2^scale vertices with ids 0..n-1, m = edgefactor * n directed edges, seeded and
 * bit-identical to oracle/jg_oracle.c:jo_rmat_edges. */
int jg_graph_build_rmat(jg_ctx* ctx, int scale, int edgefactor, uint64_t seed, uint32_t flags,
                        jg_graph** out);
int jg_graph_info_get(const jg_graph* g, jg_graph_info* out);
int jg_graph_destroy(jg_graph* g);

/* ---- programs ---- */
/* JanusGraph PageRankVertexProgram: `iterations` = maxIterations K (supersteps 0..K, i.e. K-1 power
 * steps), `vertex_count` = the user-supplied vertexCount N (NOT |V|).  rank_out[n] / edge_count_out[n]
 * (nullable) receive janusgraph.pageRank.pageRank / .edgeCount; with K == 0 no property is written
 * and rank_out is filled with NaN. */
int jg_pagerank(jg_graph* g, double damping, int64_t vertex_count, int32_t iterations,
                double* rank_out, double* edge_count_out);
/* The same run split for benchmarking: begin = supersteps 0 and 1, step = `nsteps` power supersteps
 * enqueued asynchronously, end = synchronise + copy results (either pointer nullable). */
int jg_pagerank_begin(jg_graph* g, double damping, int64_t vertex_count);
int jg_pagerank_step(jg_graph* g, int32_t nsteps);
int jg_pagerank_end(jg_graph* g, double* rank_out, double* edge_count_out);

/* The k highest-ranked vertices of the PageRank session the graph holds, selected on the device: what a
 * PageRankMapReduce emission of n (vertex id, rank) pairs
 * (janusgraph-backend-testutils/.../olap/PageRankMapReduce.java:62-67) followed by an ordering on the host
 * computes, without the two n-element arrays of jg_pagerank_end crossing to the host.
 *   Session: a jg_pagerank_begin plus any number of jg_pagerank_step calls, before or after jg_pagerank_end;
 *     a jg_pagerank with iterations >= 1 also counts (begin, step, end).  A jg_pagerank with iterations == 0
 *     runs nothing and leaves the held session, if any, as it was.  No session: JG_ERR_STATE.
 *   Lists the first min(k, n) vertices of this total order: rank descending by numeric value, ties by the
 *     caller-order index ascending (the order vid[] / the kept rows were given).  -0.0 orders as +0.0; a NaN
 *     rank (a NaN damping) orders below every number and ties with other NaNs.  Ranks are only ordered, never
 *     altered: the listed rank is the stored bit pattern.  k < 1: JG_ERR_ARG.
 *   The call runs on the shards' streams behind the steps already enqueued and does not end or disturb the
 *     session: steps may follow, and a later jg_pagerank_top sees the later ranks.  Straight after
 *     jg_pagerank_begin every rank is 1/N, so it lists the indices 0 .. k-1.
 *   num_listed_out = min(k, n); select_ms_out = HIP-event time of the select, order and emit kernels on the
 *     first shard's stream.  Both nullable.  Stats of the call (a fresh jg_stats): compute_ms = the same
 *     span, kernel_launches = the select's launches, algorithmic_bytes = its byte model (jg_top.hip).
 *   Graphs of several in-process shards (jg_ctx_create with ndev > 1, a device listed more than once
 *     included) are supported: each shard selects its own min(k, rows) and the records are merged on the
 *     host.  Rank mode (jg_ctx_create_rank*): JG_ERR_UNSUPPORTED; callers fall back to jg_pagerank_end and
 *     order on the host.
 * The list stays with the graph until the next jg_pagerank_top, jg_pagerank_top_release or jg_graph_destroy;
 * later steps, a new jg_pagerank_begin or any other program do not disturb it (it owns its storage).  A
 * failed jg_pagerank_top leaves nothing held. */
int jg_pagerank_top(jg_graph* g, int64_t k, int64_t* num_listed_out, double* select_ms_out);
/* Listed records [first, first + count): vid_out[count] = the vertex ids, index_out[count] = their
 * caller-order indices, rank_out[count] = janusgraph.pageRank.pageRank, edge_count_out[count] =
 * janusgraph.pageRank.edgeCount (the out-degree as a double, as jg_pagerank_end returns it).  Each pointer
 * nullable (a Java direct buffer holds 2 GiB, so a caller reads a large list in ranges).  Nothing held:
 * JG_ERR_STATE; a range outside [0, num_listed]: JG_ERR_ARG. */
int jg_pagerank_top_read(jg_graph* g, int64_t first, int64_t count, int64_t* vid_out, int64_t* index_out,
                         double* rank_out, double* edge_count_out);
/* Drops the held list (JG_OK when none is held). */
int jg_pagerank_top_release(jg_graph* g);

/* ShortestDistanceVertexProgram: dist_out[v] = min over paths v -> ... -> seed of <= max_depth hops
 * of the summed edge weights (int64; weights may be negative), or JG_DIST_ABSENT where Fulgora leaves
 * DISTANCE absent.  A weight of JG_WEIGHT_ABSENT marks an edge without the weight property: if a
 * message crosses one, the run fails with JG_ERR_ARG (Fulgora's edge function throws there,
 * ShortestDistanceVertexProgram.java:69); untraversed ones are harmless. */
#define JG_DIST_ABSENT INT64_MIN
#define JG_WEIGHT_ABSENT INT32_MIN
int jg_shortest_distance(jg_graph* g, int64_t seed_vid, int32_t max_depth, int64_t* dist_out);

/* Hop depth from each of nsrc sources (nsrc <= 64 runs as one bit-parallel multi-source BFS);
 * depth_out[s * n + v] = hops or -1 (unreached / beyond max_depth; max_depth < 0 = unbounded).
 * depth_out may be NULL (benchmarking: results stay on the device). */
int jg_bfs(jg_graph* g, const int64_t* source_vids, int32_t nsrc, int32_t direction,
           int32_t max_depth, int32_t* depth_out);

/* The same traversal with one output row per source: depth_rows[s] (nullable, and the array itself)
 * receives n int32 depths.  A Java direct buffer holds at most 2 GiB, so the 64 rows of one
 * bit-parallel batch cannot share one buffer past 2^23 vertices (ShortestPathVertexProgram batches,
 * java/.../GpuGraphComputer.java ShortestPaths). */
int jg_bfs_rows(jg_graph* g, const int64_t* source_vids, int32_t nsrc, int32_t direction, int32_t max_depth,
                int32_t* const* depth_rows);

/* The same traversal (nsrc <= 64: one bit-parallel batch) with its depth rows kept on the device;
 * jg_bfs_kept_row(g, s, depth_out) then copies row s (n int32, caller order) into a caller buffer, so a
 * caller that consumes the rows one at a time holds one n-int32 buffer instead of nsrc of them
 * (ShortestPathVertexProgram's batches at n = 2^26: one 268 MB row instead of 17 GB of direct buffers,
 * java/.../GpuGraphComputer.java ShortestPaths).  The rows stay until the next jg_bfs_keep, until
 * jg_bfs_kept_release or until jg_graph_destroy; jg_bfs_kept_row fails with JG_ERR_ARG for s outside
 * [0, nsrc of the last jg_bfs_keep).  Replaces FulgoraVertexMemory's per-vertex path state
 * (graphdb/olap/computer/FulgoraVertexMemory.java:52-123) for the bit-parallel batch. */
int jg_bfs_keep(jg_graph* g, const int64_t* source_vids, int32_t nsrc, int32_t direction, int32_t max_depth);
int jg_bfs_kept_row(jg_graph* g, int32_t s, int32_t* depth_out);
int jg_bfs_kept_release(jg_graph* g);

/* The shortest-path predecessor DAG of kept row s (jg_bfs_keep), built on the device: what a path walk-back
 * needs, without the adjacency rows crossing to the host.  target[n] (caller order, nullable = every
 * reached vertex is a target).
 *   Vertices: the reached targets (depth >= 0; the source too when it is a target) and every vertex on a
 *     shortest path from the source to one of them.  If any target is reached the source is listed, with
 *     an empty predecessor range.  No target reached: 0 vertices, 0 entries, deepest -1, JG_OK.
 *   Order: non-increasing depth (the source last); inside one depth unspecified, but the same on every
 *     call with the same arguments.
 *   Predecessors of v at depth d: its distinct neighbours u with depth[u] == d - 1, each once, in the
 *     order jg_graph_neighbors returns them, first occurrence kept (a multi-edge counts once, a self-loop
 *     never).  The adjacency read is the reverse of the kept traversal's: JG_DIR_BOTH reads BOTH, a
 *     JG_DIR_OUT traversal reads IN, a JG_DIR_IN traversal reads OUT; JG_ERR_UNSUPPORTED if it was not built.
 *   deepest_out: the largest depth of a reached target.  All three outputs are nullable.
 * The DAG stays with the graph until the next jg_bfs_kept_dag, jg_bfs_keep, jg_bfs_kept_release or
 * jg_graph_destroy.  s outside [0, nsrc of the last jg_bfs_keep): JG_ERR_ARG.  One shard only: graphs of
 * several shards (logical shards, rank mode) get JG_ERR_UNSUPPORTED and walk back on the host
 * (jg_bfs_kept_row + jg_graph_neighbors).  Stats: compute_ms = the DAG build (HIP events; the target mask's
 * copy in and the read-back are outside), levels = deepest, edges_traversed = the summed row lengths of the
 * DAG vertices of depth >= 1, kernel_launches = launches of the walk kernels. */
int jg_bfs_kept_dag(jg_graph* g, int32_t s, const uint8_t* target, int64_t* num_vertices_out,
                    int64_t* num_entries_out, int32_t* deepest_out);
/* DAG vertices [first, first + count): vertex_out[count] caller-order indices, depth_out[count],
 * off_out[count + 1] ABSOLUTE offsets into the DAG's predecessor array, pred_out = its entries
 * [off[first], off[first + count]) as caller-order indices.  Each pointer nullable (size first, then fill;
 * a Java direct buffer holds 2 GiB, so a caller reads a large DAG in ranges).  No DAG held (never built, or
 * dropped by a later jg_bfs_keep / jg_bfs_kept_release): JG_ERR_STATE; a range outside [0, num_vertices]:
 * JG_ERR_ARG. */
int jg_bfs_kept_dag_read(jg_graph* g, int64_t first, int64_t count, int32_t* vertex_out, int32_t* depth_out,
                         int64_t* off_out, int32_t* pred_out);
/* The edge-listing predecessor DAG of kept row s (ShortestPathVertexProgram's includeEdges: a path is
 * v, e, v, ..., v and two parallel edges give two paths).  Arguments, preconditions, the backward sweep, the DAG's
 * vertices, their order and depths, deepest and the stats are jg_bfs_kept_dag's on the same inputs.  The entries
 * differ: those of v at depth d are one per entry (u, e) of v's row in the reverse adjacency with
 * depth[u] == d - 1, in row order (the order jg_graph_neighbors / jg_graph_neighbor_edges return them): parallel
 * edges each get their own entry, a self-loop never qualifies.  num_entries_out counts them.
 * The DAG occupies jg_bfs_kept_dag's slot: either call replaces what the other held.  jg_bfs_kept_dag_read works
 * on both kinds (here pred_out repeats u once per parallel edge); jg_bfs_kept_dag_read_edges returns
 * edge_out = the edge ordinals of entries [off[first], off[first + count]), parallel to pred_out.  On a plain
 * DAG or with none held: JG_ERR_STATE; a range outside [0, num_vertices]: JG_ERR_ARG.  A graph built without
 * JG_ADJ_EDGE_INDEX: JG_ERR_UNSUPPORTED from both calls. */
int jg_bfs_kept_dag_edges(jg_graph* g, int32_t s, const uint8_t* target, int64_t* num_vertices_out,
                          int64_t* num_entries_out, int32_t* deepest_out);
int jg_bfs_kept_dag_read_edges(jg_graph* g, int64_t first, int64_t count, uint32_t* edge_out);

/* Weighted single-source shortest distances whose distance plane stays on the device (ShortestPathVertexProgram
 * with a distanceProperty): dist[v] = the smallest summed weight of a path source -> v whose edges are followed
 * in `direction`: JG_DIR_OUT along u->v (relaxes the OUT adjacency), JG_DIR_IN against u->v (the IN adjacency:
 * what jg_shortest_distance computes from its seed with an unbounding max_depth), JG_DIR_BOTH either way (the
 * BOTH adjacency built with JG_ADJ_WEIGHT_BOTH).  The engine is jg_shortest_distance's near-far delta-stepping.
 *   Preconditions: every weight of the relaxed adjacency is >= 1 (a weight <= 0 anywhere in it: JG_ERR_ARG;
 *     zero-weight edges would make the tight-edge graph of jg_sssp_kept_dag cyclic); a JG_WEIGHT_ABSENT entry
 *     that a relaxation crosses: JG_ERR_ARG, as in jg_shortest_distance.  A graph without weights, or without
 *     the relaxed adjacency (JG_DIR_BOTH: without JG_ADJ_WEIGHT_BOTH): JG_ERR_UNSUPPORTED.  A bad direction:
 *     JG_ERR_ARG.  An unknown source_vid: every distance absent, JG_OK.
 *   The plane stays with the graph until the next jg_sssp_keep, jg_sssp_kept_release or jg_graph_destroy; it is
 *     independent of jg_bfs_keep's rows and DAG (neither family drops the other's holdings).  A failed
 *     jg_sssp_keep holds nothing.
 *   jg_sssp_kept_row copies it out: dist_out[n] int64 in caller order, JG_DIST_ABSENT = unreached; nothing
 *     kept: JG_ERR_STATE.  jg_sssp_kept_release drops the plane and its DAG (JG_OK when none is held).
 *   One shard only: graphs of several shards (logical shards, rank mode) get JG_ERR_UNSUPPORTED.
 *   Stats: compute_ms = up to the distances being final on the device (HIP events), levels = near passes. */
int jg_sssp_keep(jg_graph* g, int64_t source_vid, int32_t direction);
int jg_sssp_kept_row(jg_graph* g, int64_t* dist_out);
int jg_sssp_kept_release(jg_graph* g);

/* The minimum-weight-path predecessor DAG of the kept distance plane (jg_sssp_keep), built on the device: as
 * jg_bfs_kept_dag with distance in place of depth.  target[n] (caller order, nullable = every such vertex).
 *   Targets: vertices with a present distance, <= max_distance when max_distance >= 0, and target[] set.
 *   Vertices: the targets and every vertex on a minimum-weight path from the source to one of them.  If any
 *     target is reached the source is listed last, with an empty predecessor range.  No target reached: 0
 *     vertices, 0 entries, farthest -1, JG_OK.
 *   Order: non-increasing distance; inside one distance unspecified, but the same on every call with the same
 *     arguments.
 *   Predecessors of v: its distinct neighbours u in the reverse adjacency with dist[u] present and
 *     dist[u] + w(u,v) == dist[v] (a tight edge), each once, in the order jg_graph_neighbors returns them for
 *     the reverse direction, first qualifying occurrence kept.  Of parallel edges only the lightest can be
 *     tight; with weights >= 1 a self-loop never is.  The adjacency read is the reverse of the kept
 *     direction's: JG_DIR_BOTH reads BOTH, JG_DIR_OUT reads IN, JG_DIR_IN reads OUT; JG_ERR_UNSUPPORTED if it
 *     was not built (with weights).
 *   farthest_out: the largest distance of a target.  All three outputs are nullable.
 * The DAG has its own buffers (a jg_bfs_kept_dag DAG may be held at the same time) and stays with the graph
 * until the next jg_sssp_kept_dag, jg_sssp_keep, jg_sssp_kept_release or jg_graph_destroy.  No plane kept:
 * JG_ERR_STATE.  Stats: compute_ms = the DAG build (the target mask's copy in and the read-back are outside),
 * levels = the backward sweep's rounds that had rows, edges_traversed = the summed row lengths of the DAG
 * vertices but the source, kernel_launches = launches of the walk kernels. */
int jg_sssp_kept_dag(jg_graph* g, const uint8_t* target, int64_t max_distance /* < 0: none */,
                     int64_t* num_vertices_out, int64_t* num_entries_out, int64_t* farthest_out);
/* DAG vertices [first, first + count), as jg_bfs_kept_dag_read with dist_out[count] int64 distances.  No DAG
 * held: JG_ERR_STATE; a range outside [0, num_vertices]: JG_ERR_ARG. */
int jg_sssp_kept_dag_read(jg_graph* g, int64_t first, int64_t count, int32_t* vertex_out, int64_t* dist_out,
                          int64_t* off_out, int32_t* pred_out);
/* The edge-listing twin of jg_sssp_kept_dag, as jg_bfs_kept_dag_edges is of jg_bfs_kept_dag: the entries of v
 * are one per entry (u, e) of its reverse row with dist[u] present and dist[u] + w(e) == dist[v], in row order
 * (of parallel edges every lightest one; a heavier one is not tight).  It occupies jg_sssp_kept_dag's slot;
 * jg_sssp_kept_dag_read works on both kinds, jg_sssp_kept_dag_read_edges returns the ordinals.  Errors as for
 * the jg_bfs_kept_dag_edges pair. */
int jg_sssp_kept_dag_edges(jg_graph* g, const uint8_t* target, int64_t max_distance /* < 0: none */,
                           int64_t* num_vertices_out, int64_t* num_entries_out, int64_t* farthest_out);
int jg_sssp_kept_dag_read_edges(jg_graph* g, int64_t first, int64_t count, uint32_t* edge_out);

/* ---- the same over double edge weights (ShortestPathVertexProgram with a Double distanceProperty) ----
 *
 * Distance.  A path's length is the IEEE-754 binary64 sum of its edges' weights, added left to right from the
 *   source, starting from +0.0; dist[v] is the smallest such sum.  fl(a + w) is monotone in a, so this is the
 *   fixed point dist[v] = min over u of fl(dist[u] + w(u,v)) that the relaxation reaches, and what a host
 *   Dijkstra over doubles computes, bit for bit.  Distances are held as their bit patterns: a non-negative
 *   double read as a signed 64-bit integer orders as its value does, so the engine relaxes with the integer
 *   atomicMin of jg_sssp_keep; no float atomic is used and nothing depends on arrival order.
 * Tight edges.  u -> v with weight w is tight iff dist[u] is present, fl(dist[u] + w) == dist[v] as doubles and
 *   dist[u] < dist[v].  No epsilon: 0.25 + 0.25 ties with a direct 0.5; 0.1 + 0.2 loses to a direct 0.3.
 * Unreached: JG_DISTF_ABSENT (+Inf) in every double output.
 *
 * jg_graph_set_weights_f64: weight[m] = one double per edge of the edge list the graph was built from, in that
 *   list's order.  The graph must have been built from ids (jg_graph_build, or a builder fed vertex / edge ids)
 *   with JG_ADJ_EDGE_INDEX, hence on one shard; any other graph: JG_ERR_UNSUPPORTED.  m other than that list's
 *   length, or a null array with m > 0: JG_ERR_ARG.  The array is uploaded, checked by one device reduction in a
 *   fixed order (per-workgroup partials summed in workgroup order: the same statistics, automatic delta and
 *   stats.levels on every run), and gathered beside every adjacency that was built (8 bytes per entry, counted
 *   in jg_graph_info.device_bytes).
 *     Every weight must be finite and > 0, else JG_ERR_ARG.
 *     No relaxation may be absorbed (dist + w == dist would make the tight-edge graph cyclic): with rows = the
 *     vertex count, wmin >= rows * wmax * 2^-52, wmin >= DBL_MIN and rows * wmax finite are required, else
 *     JG_ERR_UNSUPPORTED (callers delegate).  Under that gate every relaxed edge strictly increases the distance
 *     and no stored distance is infinite (jg_sssp.hip states the argument).
 *   A second call replaces the weights and drops a kept f64 plane and its DAG; a failed call leaves the graph as
 *   it was.  The int32 weights of the build, if any, are untouched.
 * jg_sssp_keep_f64: jg_sssp_keep over those weights; direction, unknown source, stats and the one-shard rule as
 *   there.  No absent marker exists on this route.  Without jg_graph_set_weights_f64, or without the relaxed
 *   adjacency: JG_ERR_UNSUPPORTED.  JG_DIR_BOTH needs JG_ADJ_BOTH only (the doubles are gathered onto both
 *   entries of an edge; JG_ADJ_WEIGHT_BOTH is not needed).  The automatic delta is 128 x the mean weight / the mean
 *   degree, in double, at least wmin.  Its near passes relax each queued row from its distance as it stood
 *   before the pass, so the plane and stats.levels (the near passes) are the same on every run; a threshold
 *   change first tries T + delta and jumps to the far pile's exact minimum only when that bucket was empty.
 *   The plane takes jg_sssp_keep's slot: a keep of
 *   either kind drops the other's plane and DAG, jg_sssp_kept_release drops either.
 * jg_sssp_kept_row_f64: dist_out[n] doubles in caller order.
 * jg_sssp_kept_dag_f64 / jg_sssp_kept_dag_edges_f64 / jg_sssp_kept_dag_read_f64: as the integer calls, with the
 *   tight-edge rule above.  max_distance is inclusive on the sum; < 0 or NaN: none.  farthest_out: -1.0 when no
 *   target is reached.  Predecessors of v: each u with a tight entry once, at its first tight entry, in the
 *   reverse row's order; the edge-listing twin lists every tight entry.  jg_sssp_kept_dag_read_edges serves both
 *   kinds of edge-listing DAG.
 * Kinds do not mix: jg_sssp_kept_row, jg_sssp_kept_dag, jg_sssp_kept_dag_edges on an f64 plane,
 *   jg_sssp_kept_dag_read on an f64 DAG, and the _f64 calls on an integer plane or DAG: JG_ERR_STATE.
 * Not covered (callers delegate): Float (binary32) properties, whose sums TinkerPop takes in float arithmetic;
 *   Long weights beyond int32; graphs of several shards; graphs built from rows (the decoder skips doubles). */
#define JG_DISTF_ABSENT (__builtin_huge_val()) /* +Inf (gcc, clang) */
int jg_graph_set_weights_f64(jg_graph* g, const double* weight, int64_t m);
int jg_sssp_keep_f64(jg_graph* g, int64_t source_vid, int32_t direction);
int jg_sssp_kept_row_f64(jg_graph* g, double* dist_out);
int jg_sssp_kept_dag_f64(jg_graph* g, const uint8_t* target, double max_distance /* < 0 or NaN: none */,
                         int64_t* num_vertices_out, int64_t* num_entries_out, double* farthest_out);
int jg_sssp_kept_dag_edges_f64(jg_graph* g, const uint8_t* target, double max_distance /* < 0 or NaN: none */,
                               int64_t* num_vertices_out, int64_t* num_entries_out, double* farthest_out);
int jg_sssp_kept_dag_read_f64(jg_graph* g, int64_t first, int64_t count, int32_t* vertex_out, double* dist_out,
                              int64_t* off_out, int32_t* pred_out);

/* Adjacency of vertices rows[0, nrows) (output-order indices), in output-order indices: the host copy
 * of the snapshot a path walk-back reads where Fulgora re-reads each vertex's preloaded BOTH slice
 * (graphdb/olap/computer/VertexProgramScanJob.java:113-135).  direction JG_DIR_BOTH (a self-loop
 * appears twice, multi-edges repeat), JG_DIR_OUT or JG_DIR_IN (the adjacency must have been built).
 * off_out[nrows + 1] = exclusive prefix of the rows' entry counts; nbr_out[off_out[nrows]] (nullable:
 * size first, then fill) = the neighbours.  Rank mode (jg_ctx_create_rank*): entry counts only
 * (nbr_out must be NULL, else JG_ERR_UNSUPPORTED), and rows of other ranks count 0 entries. */
int jg_graph_neighbors(const jg_graph* g, int32_t direction, const int64_t* rows, int64_t nrows, int64_t* off_out,
                       int64_t* nbr_out);
/* The edge ordinals (JG_ADJ_EDGE_INDEX) of the same entries: same rows, same off_out, same size-first-then-fill
 * rule; edge_out[i] is the ordinal of the entry whose neighbour jg_graph_neighbors reports at i.  A graph built
 * without the flag: JG_ERR_UNSUPPORTED. */
int jg_graph_neighbor_edges(const jg_graph* g, int32_t direction, const int64_t* rows, int64_t nrows,
                            int64_t* off_out, uint32_t* edge_out);

/* ConnectedComponentVertexProgram: component_vid_out[v] = the vertex id whose decimal String is the
 * component label (the String-minimum id of v's weakly connected component).  iterations_out
 * (nullable) = supersteps of the synchronous program. */
int jg_connected_components(jg_graph* g, int64_t* component_vid_out, int32_t* iterations_out);

/* The component census of ConnectedComponentVertexProgram, made on the device: what TinkerPop's
 * ClusterCountMapReduce / ClusterPopulationMapReduce (group().by(component).by(count())) compute from the
 * program's result, without the n component ids crossing to the host.  jg_cc_census runs the program exactly
 * as jg_connected_components(g, NULL, iterations_out) does (same path selection: union-find, propagation,
 * the 99-superstep cap; same labels, same iterations_out) and then counts the vertices of each label there.
 *   Component: a distinct label of the run, i.e. the vertex id whose decimal String is the minimum of the
 *     component; its population = the vertices carrying that label.  A vertex without edges is its own
 *     component of population 1.  When the 99-superstep cap binds, the census is of the labels the program
 *     returns (what jg_connected_components would hand back), not of the true components.
 *   num_components_out = all components; largest_out = the largest population (0 if the graph has no
 *     vertex); num_listed_out = the components with population >= min_population: only these are held for
 *     jg_cc_census_read.  min_population < 1: JG_ERR_ARG.  A min_population above the largest population
 *     lists nothing and returns JG_OK.  Every output pointer is nullable.
 *   Order of the listed components: population descending, ties by the label's decimal String ascending
 *     (String.compareTo); the same on every call.
 *   census_ms_out = HIP-event time of the census kernels alone.  Stats of the call: supersteps, levels and
 *     edges_traversed as jg_connected_components reports them; compute_ms = the whole device span (the
 *     program and the census); algorithmic_bytes = the program's model + the census's (jg_census.hip).
 *   Errors as for jg_connected_components: JG_ERR_UNSUPPORTED for a graph built without JG_ADJ_BOTH or with
 *     negative vertex ids.  One shard only: graphs of several shards (logical shards, rank mode) get
 *     JG_ERR_UNSUPPORTED; callers fall back to jg_connected_components and group on the host.
 * The census stays with the graph until the next jg_cc_census, jg_cc_census_release or jg_graph_destroy; a
 * jg_connected_components, a traversal or any other program in between does not disturb it (it owns its
 * buffers).  A failed jg_cc_census leaves no census held. */
int jg_cc_census(jg_graph* g, int64_t min_population, int32_t* iterations_out, int64_t* num_components_out,
                 int64_t* num_listed_out, int64_t* largest_out, double* census_ms_out);
/* Listed components [first, first + count): component_vid_out[count] = their ids (vertex ids, as
 * jg_connected_components returns them), population_out[count] = their populations.  Each pointer nullable
 * (a Java direct buffer holds 2 GiB, so a caller reads a large census in ranges).  No census held:
 * JG_ERR_STATE; a range outside [0, num_listed]: JG_ERR_ARG. */
int jg_cc_census_read(jg_graph* g, int64_t first, int64_t count, int64_t* component_vid_out,
                      int64_t* population_out);
/* Drops the held census (JG_OK when none is held). */
int jg_cc_census_release(jg_graph* g);

/* PeerPressureVertexProgram (TinkerPop 3.4.6, g.V().peerPressure(); third party, recalled): every vertex
 * starts in its own cluster (cluster id = its vertex id) and repeatedly joins the cluster that its neighbours
 * vote for most strongly.  cluster_vid_out[n] (caller order, nullable) = the id of each vertex's cluster.
 *   direction = the edges of the vote scope.  JG_DIR_OUT (the program's default, outE): a vertex votes along its
 *     out-edges, so vertex v receives one vote per entry of its IN adjacency row (the pull of
 *     VertexMemoryHandler.java:121-151; multi-edges count once per edge).  JG_DIR_BOTH (bothE): v receives one
 *     vote per entry of its BOTH row (a self-loop appears twice).
 *   Strength: distribute_vote == 0: every vote weighs 1.  distribute_vote != 0: the vote of u weighs
 *     1.0 / (number of entries in which u is the sender) as an IEEE double: u's out-degree under JG_DIR_OUT, the
 *     length of its BOTH row under JG_DIR_BOTH; a vertex that is the sender of no entry has strength +Inf, sends
 *     nothing and never leaves its own cluster.
 *   Vote superstep (synchronous: every read is of the previous superstep): votes = {cluster[v]: strength[v]},
 *     then votes[cluster[u]] += strength[u] for every entry u of v's row; v's new cluster is the one with the
 *     largest sum.  Sums are fp64; the order of the additions inside one sum is unspecified, but the result is
 *     the same on every run over the same graph.
 *   Tie rule (this library's own): among clusters with exactly equal sums the numerically smallest cluster id
 *     (signed int64) wins.  Fulgora's choice in a tie follows HashMap iteration order and message arrival order;
 *     no caller can rely on it.
 *   Halting: vote supersteps run until one changes no vertex's cluster or max_iterations of them have run
 *     (0 is legal: every vertex keeps its own id; < 0: JG_ERR_ARG).  iterations_out (nullable) =
 *     memory().getIteration() of the Fulgora run (FulgoraGraphComputer.java:210-230, whose incrIteration also runs
 *     on the terminating pass) = vote supersteps executed + 1, + 1 more with distribute_vote (the counting
 *     superstep).
 *   Errors: JG_DIR_OUT needs JG_ADJ_IN at build time, JG_DIR_BOTH needs JG_ADJ_BOTH, else JG_ERR_UNSUPPORTED.
 *     JG_DIR_IN is JG_ERR_UNSUPPORTED: its vote strength divides by an in-degree, and a graph built with
 *     JG_ADJ_OUT alone (the adjacency it would pull over) holds none.  One shard only: graphs of several shards
 *     (logical shards, rank mode) get JG_ERR_UNSUPPORTED.
 *   Stats: supersteps = iterations; levels = vote supersteps executed; compute_ms = the whole device run (HIP
 *     events); kernel_ms_total / kernel_launches = the vote kernels alone; edges_traversed = vote supersteps x
 *     entries of the adjacency read; algorithmic_bytes = the byte model of jg_peer.hip.
 * Holds nothing afterwards and disturbs no held census, kept traversal or PageRank session. */
int jg_peer_pressure(jg_graph* g, int32_t direction /* JG_DIR_OUT | JG_DIR_BOTH: the vote scope's edges */,
                     int32_t distribute_vote, int32_t max_iterations,
                     int64_t* cluster_vid_out /* [n], caller order, nullable */, int32_t* iterations_out /* nullable */);

/* Combiner vertex programs (the DegreeCounter family, janusgraph-test/.../olap/OLAPTest.java:424-503):
 * x_0 = init[v] (NULL: every vertex sends 1), then `steps` supersteps of
 *     x_t[v] = COMBINE over the entries (v, w) of v's `direction` adjacency of x_{t-1}[w]
 * (JG_DIR_OUT: v's out-edges, i.e. messages sent on Local.of(inE); one term per edge).  COMBINE is
 * JG_COMBINE_SUM (a vertex with no entries gets 0, as reduce(0, +)), _MIN or _MAX (no entries: the
 * identity, and received_out[v] = 0).  int32_wrap != 0: Java Integer values (inputs truncated to
 * int32, sums modulo 2^32).  out[n] = x_steps; received_out[n] (nullable) = v had at least one term
 * in the last superstep.  Needs the matching adjacency at build time; sharded graphs exchange the messages every superstep. */
#define JG_COMBINE_SUM 0
#define JG_COMBINE_MIN 1
#define JG_COMBINE_MAX 2
int jg_combine_steps(jg_graph* g, int32_t direction, int32_t combiner, int32_t int32_wrap, const int64_t* init,
                     int32_t steps, int64_t* out, uint8_t* received_out);

/* Decode n edgestore entries on the context's first GPU, as EdgeSerializer.parseRelation does
 * (core/graphdb/database/EdgeSerializer.java:86-122; header: IDHandler.readRelationType,
 * idhandling/IDHandler.java:130-141; varints: idhandling/VariableLong.java:44-52,193-208,276-294).
 * Entry i is bytes[entry_off[i] .. entry_off[i+1]) (column then value), value_pos[i] its value
 * position (the column length).  type_ids / type_mult (ntypes, may be 0) give the multiplicity of
 * edge labels: 0 MULTI, 1 SIMPLE, 2 ONE2MANY, 3 MANY2ONE, 4 ONE2ONE (core/core/Multiplicity.java);
 * labels absent from the table are MULTI.  Outputs per entry (each nullable): the relation type id,
 * dir_out = 0 OUT edge, 1 IN edge, 2 property, 3 system relation, -1 malformed; the other vertex id
 * and the relation id (-1 unless a user edge).  Stats: compute_ms = kernel time. */
int jg_decode_edges(jg_ctx* ctx, const uint8_t* bytes, int64_t nbytes, const int64_t* entry_off,
                    const int32_t* value_pos, int64_t n, const int64_t* type_ids, const int8_t* type_mult,
                    int32_t ntypes, int64_t* type_out, int8_t* dir_out, int64_t* other_out, int64_t* relation_out);

/* Block until all work enqueued on the graph's streams is complete. */
int jg_graph_sync(jg_graph* g);

/* Process-wide performance knobs (no effect on results).  Every key, its default and the measurement
 * behind it is in `struct Tune` (janusgraph_amd/csrc/jg_internal.h); the ranges are checked here:
 *   0/1 switches (any other value: JG_ERR_ARG): "pull_split", "halo" (read at build; sharded graphs:
 *     0 = dense allgather), "bfs_narrow", "cc_push", "cc_uf", "cc_uf_sharded", "cc_uf_search",
 *     "cc_sparse", "msbfs_sparse", "msbfs_skip", "msbfs_split", "sharded_bfs";
 *   integers: "bfs_alpha", "dobfs_alpha", "bfs_beta", "nb_alpha" [1, 1e6]; "nb_first" [4, 4096];
 *     "msbfs_td" [0, 2]; "msbfs_exit" [0, 2]; "cc_first" [1, 64]; "msbfs_td_rowapply" [0, 1024];
 *     "msbfs_td_noprobe", "msbfs_exit_live" [0, 1000]; "msbfs_scan_queue" [0, 1001];
 *     "msbfs_exit_first" [1, 256]; "bfs_td_split" [0, 2]; "bfs_td_split_levels" [0, 0xffff];
 *     "bfs_td_split_min" / "_max" [1, 2^31); "bfs_batch0" [1, 64]; "bfs_grid_mult" [1, 64];
 *     "bfs_grid" [64, 65536]; "bfs_tail_grid" [0, 65536]; "merge_temporal" [0, 2];
 *     "merge_hot" [-1, 2^30]; "merge_off32" [0, 1];
 *     "sd_delta" [-1, 2^30]; "sd_dist32" [0, 2]; "merge_pack" 0 | 1 | 24; "merge_stage<i>" -1 | 0 | 64 | 128 | 256 | 512;
 *     read at build: "band<i>_deg" (>= -1), "band<i>_bit" (0 or [3, 8]), "band<i>_sub" (power of two <= 256);
 *     "edgestore_chunk_entries", "edgestore_chunk_bytes" (>= 1): the chunk limits of jg_graph_build_edgestore
 *     (tests lower them; rows never split, so a larger row is a chunk of its own);
 *   retired (their variants were measured slower and removed; accepted and ignored): "pull_unroll",
 *     "pull_nt", "pull_lds", "light_lds", "slice_lds", "pull_short", "pull_overlap", "bfs_persistent".
 * Unknown key or value out of range: JG_ERR_ARG. */
int jg_tune_set(const char* key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* JANUSGPU_H */
