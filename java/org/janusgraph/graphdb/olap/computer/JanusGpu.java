// Copyright 2026 JanusGraph Authors
// SPDX-License-Identifier: Apache-2.0
package org.janusgraph.graphdb.olap.computer;

import org.janusgraph.core.JanusGraphException;

import java.nio.ByteBuffer;

/**
 * JNI binding of libjanusgpu (include/janusgpu.h). Every native method returns the C status code
 * (0 = ok, &lt; 0 = error class); {@link #check(int)} turns a failure into a JanusGraphException
 * carrying jg_last_error(), in the style of FulgoraGraphComputer's "Computer is aborting" errors
 * (janusgraph-core/.../olap/computer/FulgoraGraphComputer.java:269-286).
 *
 * Arrays cross the boundary as direct ByteBuffers in native byte order (int64 ids and offsets, int32
 * weights / value positions, float64 / int64 outputs); handles are opaque longs. A direct buffer
 * holds at most 2 GiB, so snapshots go through the chunked builder (jg_builder_*) and outputs are
 * per-vertex arrays (n * 8 bytes). Java 8 target (pom.xml:112-113): JNI, not Panama.
 */
final class JanusGpu {
    /** JG_ABI_VERSION of include/janusgpu.h that these natives and their array layouts follow. */
    static final int ABI_VERSION = 3;

    static {
        System.loadLibrary("janusgpu_jni"); // links libjanusgpu.so
        if (abiVersion() != ABI_VERSION)
            throw new ExceptionInInitializerError("libjanusgpu ABI " + abiVersion() + ", GpuGraphComputer needs "
                + ABI_VERSION + ": rebuild libjanusgpu and libjanusgpu_jni");
    }

    static final int ADJ_OUT = 1, ADJ_IN = 2, ADJ_BOTH = 4;
    static final int DIR_OUT = 1, DIR_IN = 2, DIR_BOTH = 3;
    static final long DIST_ABSENT = Long.MIN_VALUE;    // JG_DIST_ABSENT
    static final int WEIGHT_ABSENT = Integer.MIN_VALUE; // JG_WEIGHT_ABSENT

    private JanusGpu() {
    }

    static native int abiVersion();
    static native String lastError();

    /** jg_ctx_create(devices, ndev, &ctx); handle written to out[0]. */
    static native int ctxCreate(int[] devices, long[] out);
    static native int ctxDestroy(long ctx);
    /** jg_ctx_trim: the device memory libjanusgpu caches for reuse goes back to the devices. */
    static native int ctxTrim(long ctx);
    /** jg_ctx_last_stats: supersteps, levels, build_ms, compute_ms, exchange_ms, kernel_ms, launches, bytes, edges. */
    static native int ctxLastStats(long ctx, double[] out9);

    /** jg_builder_create; handle written to out[0]. */
    static native int builderCreate(long ctx, long[] out);
    static native int builderDestroy(long builder);
    static native int builderAddVertices(long builder, ByteBuffer vid, long n);
    /** weight: int32 direct buffer or null (the same on every call). */
    static native int builderAddEdges(long builder, ByteBuffer src, ByteBuffer dst, ByteBuffer weight, long m);
    static native int builderSetSchema(long builder, ByteBuffer typeIds, ByteBuffer typeMult, int ntypes,
                                       int partitionBits);
    /** One scan chunk of whole rows: keys (int64), row entry offsets (int64, nrows + 1), entry bytes,
     *  entry offsets (int64, nentries + 1), value positions (int32), entry weights (int32 or null). */
    static native int builderAddRows(long builder, ByteBuffer rowKeys, long nrows, ByteBuffer rowEntryOff,
                                     ByteBuffer bytes, long nbytes, ByteBuffer entryOff, ByteBuffer valuePos,
                                     ByteBuffer entryWeight, long nentries);
    /** jg_builder_set_weight_key: the edges' Integer weight decoded on the GPU. weightKey and keyIds are inline
     *  ids (IDManager.stripRelationTypePadding), keyTypes the JG_PROP_* codes (int8). */
    static native int builderSetWeightKey(long builder, long weightKey, ByteBuffer keyIds, ByteBuffer keyTypes,
                                          int nkeys);
    /** jg_builder_set_query_limit: Fulgora's per-row slice cap (0: none); inEntries DIR_IN or DIR_OUT. */
    static native int builderSetQueryLimit(long builder, long limit, int inEntries);
    /** jg_builder_finish; graph handle written to out[0]. */
    static native int builderFinish(long builder, int flags, long[] out);
    /** jg_builder_keep_labels: a label beside every edge (before the first chunk; never with a query limit). */
    static native int builderKeepLabels(long builder);
    /** jg_builder_add_labeled_edges: builderAddEdges plus one int64 label per edge (label-keeping builders). */
    static native int builderAddLabeledEdges(long builder, ByteBuffer src, ByteBuffer dst, ByteBuffer weight,
                                             ByteBuffer label, long m);
    /** jg_builder_finish_labels: the graph of one typed scope (labels: int64 direct buffer of nlabels ids);
     *  graph handle written to out[0].  May be called again; builderFinish afterwards covers every label. */
    static native int builderFinishLabels(long builder, ByteBuffer labels, int nlabels, int flags, long[] out);

    static native int graphDestroy(long graph);
    /** jg_graph_info_get: vertices, edges, ghost edges, self loops, truncated vertices, max in, max out, bytes. */
    static native int graphInfo(long graph, long[] out8);
    /** jg_graph_vertex_ids(offset, count) into an int64 direct buffer. */
    static native int graphVertexIds(long graph, long offset, long count, ByteBuffer vidOut);

    static native int pageRank(long graph, double damping, long vertexCount, int iterations, ByteBuffer rankOut,
                               ByteBuffer edgeCountOut);
    static native int shortestDistance(long graph, long seedVid, int maxDepth, ByteBuffer distOut);
    static native int bfs(long graph, ByteBuffer sourceVids, int nsrc, int direction, int maxDepth, ByteBuffer depthOut);
    /** jg_bfs_rows: one int32 direct buffer of n depths per source (null: not wanted). */
    static native int bfsRows(long graph, ByteBuffer sourceVids, int nsrc, int direction, int maxDepth,
                              ByteBuffer[] depthRows);
    /** jg_bfs_keep: the traversal's depth rows (<= 64 sources) stay on the device for bfsKeptRow. */
    static native int bfsKeep(long graph, ByteBuffer sourceVids, int nsrc, int direction, int maxDepth);
    /** jg_bfs_kept_row: row s of the last bfsKeep into an int32 direct buffer of n depths. */
    static native int bfsKeptRow(long graph, int s, ByteBuffer depthOut);
    /** jg_bfs_kept_release: frees the kept rows before the graph goes. */
    static native int bfsKeptRelease(long graph);
    /** jg_bfs_kept_dag: builds the predecessor DAG of kept row s on the device (one shard; target: one byte
     *  per vertex, null = every reached vertex); out3 = {vertices, predecessor entries, deepest}. */
    static native int bfsKeptDag(long graph, int s, ByteBuffer target, long[] out3);
    /** jg_bfs_kept_dag_read: DAG vertices [first, first + count) into direct buffers (each nullable): int32
     *  vertices and depths, int64 absolute offsets (count + 1), int32 predecessors [off[first], off[first + count]). */
    static native int bfsKeptDagRead(long graph, long first, long count, ByteBuffer vertexOut, ByteBuffer depthOut,
                                     ByteBuffer offOut, ByteBuffer predOut);
    /** jg_graph_neighbors: rows (int64 output-order indices) -> offsets (int64, nrows + 1) and neighbours
     *  (int64 output-order indices; null: offsets only). */
    static native int graphNeighbors(long graph, int direction, ByteBuffer rows, long nrows, ByteBuffer offOut,
                                     ByteBuffer nbrOut);
    static native int connectedComponents(long graph, ByteBuffer componentVidOut, int[] iterationsOut);
    /** jg_cc_census: runs the program and counts each component's vertices on the device (one shard);
     *  out4 = {iterations, components, listed components (population >= minPopulation), largest population},
     *  censusMsOut[0] = the census kernels' time. */
    static native int ccCensus(long graph, long minPopulation, long[] out4, double[] censusMsOut);
    /** jg_cc_census_read: listed components [first, first + count), population descending, into int64 direct
     *  buffers (each nullable): the component's vertex id, its population. */
    static native int ccCensusRead(long graph, long first, long count, ByteBuffer componentVidOut,
                                   ByteBuffer populationOut);
    /** jg_cc_census_release: drops the held census before the graph goes. */
    static native int ccCensusRelease(long graph);
    /** jg_peer_pressure: PeerPressureVertexProgram on one shard over the edges direction (1 outE, 3 bothE);
     *  clusterVidOut: an int64 direct buffer of n cluster ids (null: not wanted), iterationsOut[0] =
     *  memory.getIteration().  Ties go to the numerically smallest cluster id. */
    static native int peerPressure(long graph, int direction, int distributeVote, int maxIterations,
                                   ByteBuffer clusterVidOut, int[] iterationsOut);
    /** jg_sssp_keep: the smallest summed edge weights from sourceVid along direction (1 out, 2 in, 3 both; weights
     *  >= 1, one shard), kept on the device for ssspKeptRow / ssspKeptDag. */
    static native int ssspKeep(long graph, long sourceVid, int direction);
    /** jg_sssp_kept_row: the kept distances into an int64 direct buffer of n (Long.MIN_VALUE: unreached). */
    static native int ssspKeptRow(long graph, ByteBuffer distOut);
    /** jg_sssp_kept_release: drops the kept distances and their DAG. */
    static native int ssspKeptRelease(long graph);
    /** jg_sssp_kept_dag: the minimum-weight-path predecessor DAG of the kept distances, built on the device;
     *  target: one byte per vertex (null: every reached vertex), maxDistance < 0: no bound;
     *  out3 = {vertices, predecessor entries, farthest target distance}. */
    static native int ssspKeptDag(long graph, ByteBuffer target, long maxDistance, long[] out3);
    /** jg_sssp_kept_dag_read: DAG vertices [first, first + count) into direct buffers (each nullable): int32
     *  vertices, int64 distances, int64 absolute offsets (count + 1), int32 predecessors. */
    static native int ssspKeptDagRead(long graph, long first, long count, ByteBuffer vertexOut, ByteBuffer distOut,
                                      ByteBuffer offOut, ByteBuffer predOut);
    /** jg_pagerank_top: the min(k, n) highest-ranked vertices of the held PageRank session, selected on the
     *  device (rank descending, ties by snapshot order); listedOut[0] = the records listed, selectMsOut[0] =
     *  the select's device time.  The list stays with the graph for pagerankTopRead. */
    static native int pagerankTop(long graph, long k, long[] listedOut, double[] selectMsOut);
    /** jg_pagerank_top_read: listed records [first, first + count) into direct buffers (each nullable): int64
     *  vertex ids and snapshot indices, double pageRank and edgeCount. */
    static native int pagerankTopRead(long graph, long first, long count, ByteBuffer vidOut, ByteBuffer indexOut,
                                      ByteBuffer rankOut, ByteBuffer edgeCountOut);
    /** jg_pagerank_top_release: drops the held list before the graph goes. */
    static native int pagerankTopRelease(long graph);
    /** jg_combine_steps: sum/min/max MessageCombiner programs (OLAPTest.DegreeCounter family). */
    static native int combineSteps(long graph, int direction, int combiner, int int32Wrap, ByteBuffer init, int steps,
                                   ByteBuffer out, ByteBuffer receivedOut);

    static void check(int status) {
        if (status != 0) {
            throw new JanusGraphException(
                "GPU computer is aborting: libjanusgpu status " + status + ": " + lastError());
        }
    }
}
