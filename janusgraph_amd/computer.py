"""GpuGraphComputer — host-side mirror of the TinkerPop GraphComputer API over libjanusgpu.

Mirrors FulgoraGraphComputer (janusgraph-core/src/main/java/org/janusgraph/graphdb/olap/computer/
FulgoraGraphComputer.java):
  vertices/edges (graph filters: stored, unsupported at submit)          :108-118, :522
  result/persist/workers/program/mapReduce (+ JanusGraphComputer.resultMode) :120-152
  submit(): single use, validation, async execution -> Future[ComputerResult] :154-208
  memory().getIteration() == last superstep index, getRuntime() in ms        FulgoraMemory.java:97-101
  map-reduce results under mr.memory_key                                      :288-357
  write-back of computed keys (ORIGINAL -> the graph, NEW -> a result view)   :359-471
The supersteps themselves run in libjanusgpu (HIP, gfx950): this module snapshots the graph once,
calls the C-ABI, and shapes the outputs like Fulgora's.  There is no CPU execution path: programs
the GPU does not run raise ProgramNotSupported (the Java side delegates those to Fulgora).
"""
from __future__ import annotations

import concurrent.futures as cf
import time

import numpy as np

from . import _lib
from .computer_types import (Persist, ProgramNotSupported, ResultGraph, ResultMode, computer_has_already_been_submitted,
                             computer_has_no_vertex_program_nor_map_reducers, graph_filter_not_supported)
from .graph import InMemoryGraph
from .programs import (ClusterCountMapReduce, ClusterPopulationMapReduce, CombinerVertexProgram,
                       ConnectedComponentVertexProgram, PageRankTopMapReduce, PageRankVertexProgram,
                       PeerPressureVertexProgram, ShortestDistanceVertexProgram, ShortestPathVertexProgram)


class Memory:
    """Global memory of a finished computation (FulgoraMemory after complete())."""

    def __init__(self):
        self._map = {}
        self._iteration = 0
        self._runtime = 0

    def get(self, key):
        if key not in self._map:
            raise KeyError(f"The memory does not contain the provided key: {key}")
        return self._map[key]

    def set(self, key, value):
        self._map[key] = value

    def exists(self, key):
        return key in self._map

    def keys(self):
        return set(self._map)

    def getIteration(self):  # noqa: N802
        return self._iteration

    def getRuntime(self):  # noqa: N802
        return self._runtime

    iteration = property(getIteration)
    runtime = property(getRuntime)


class ComputedGraph:
    """ResultGraph.NEW view: the original vertices with the computed keys overlaid."""

    def __init__(self, base: InMemoryGraph, props: dict):
        self.base, self.props = base, props

    def value(self, vid, key):
        return self.props[int(vid)][key]

    def properties(self, vid):
        return self.props.get(int(vid), {})


class ComputerResult:
    def __init__(self, graph, memory: Memory):
        self._graph, self._memory = graph, memory

    def graph(self):
        return self._graph

    def memory(self) -> Memory:
        return self._memory


class GpuGraphComputer:
    """graph.compute(GpuGraphComputer.class) for the programs of programs.RECOGNISED."""

    def __init__(self, graph: InMemoryGraph, devices=(0,), context: _lib.Context | None = None):
        self.graph = graph
        self.devices = tuple(devices)
        self._context = context
        self.vertex_program = None
        self.map_reduces = []
        self.result_graph_mode = None
        self.persist_mode = None
        self.num_threads = 1
        self.vertex_filter = None
        self.edge_filter = None
        self.executed = False
        self._map_reduced = False  # the vertex program's route already filled the map-reduces' memory keys

    # ---- GraphComputer builder methods ----
    def vertices(self, vertex_filter):
        self.vertex_filter = vertex_filter
        return self

    def edges(self, edge_filter):
        self.edge_filter = edge_filter
        return self

    def result(self, mode: ResultGraph):
        if mode is None:
            raise ValueError("Need to specify mode")
        self.result_graph_mode = mode
        return self

    def persist(self, mode: Persist):
        if mode is None:
            raise ValueError("Need to specify mode")
        self.persist_mode = mode
        return self

    def resultMode(self, mode: ResultMode):  # noqa: N802 (JanusGraphComputer.resultMode)
        return self.result(mode.result_graph).persist(mode.persist)

    def workers(self, threads: int):
        if threads <= 0:
            raise ValueError(f"Invalid number of threads: {threads}")
        self.num_threads = threads  # GPU parallelism is internal; accepted for API parity
        return self

    def program(self, vertex_program):
        if self.vertex_program is not None:
            raise RuntimeError("A vertex program has already been set")
        self.vertex_program = vertex_program
        return self

    def mapReduce(self, map_reduce):  # noqa: N802
        self.map_reduces.append(map_reduce)
        return self

    @staticmethod
    def features():
        return {"supportsVertexAddition": False, "supportsVertexRemoval": False,
                "supportsVertexPropertyAddition": True, "supportsVertexPropertyRemoval": False,
                "supportsEdgeAddition": False, "supportsEdgeRemoval": False, "supportsEdgePropertyAddition": False,
                "supportsEdgePropertyRemoval": False, "supportsGraphFilter": False}

    # ---- submit ----
    def submit(self) -> cf.Future:
        if self.executed:
            raise computer_has_already_been_submitted()
        self.executed = True
        if self.vertex_program is None and not self.map_reduces:
            raise computer_has_no_vertex_program_nor_map_reducers()
        if self.vertex_filter is not None or self.edge_filter is not None:
            raise graph_filter_not_supported()
        vp = self.vertex_program
        if vp is not None:
            if not isinstance(vp, (PageRankVertexProgram, ShortestDistanceVertexProgram,
                                   ConnectedComponentVertexProgram, ShortestPathVertexProgram,
                                   CombinerVertexProgram, PeerPressureVertexProgram)):
                raise ProgramNotSupported(f"{type(vp).__name__} is not run by GpuGraphComputer; "
                                          f"delegate to FulgoraGraphComputer")
            self.map_reduces.extend(vp.get_map_reducers())
        if self.persist_mode is None:
            self.persist_mode = vp.preferred_persist if vp is not None else Persist.NOTHING
        if self.result_graph_mode is None:
            self.result_graph_mode = vp.preferred_result_graph if vp is not None else ResultGraph.ORIGINAL
        pool = cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="GpuGraphComputer")
        fut = pool.submit(self._submit_async)
        pool.shutdown(wait=False)
        return fut

    # ---- execution ----
    def _ctx(self) -> _lib.Context:
        if self._context is None:
            self._context = _lib.Context(self.devices)
        return self._context

    def _submit_async(self) -> ComputerResult:
        t0 = time.perf_counter()
        memory = Memory()
        props = {}
        vids = None
        if self.vertex_program is not None:
            vids, props, iteration, extra = self._execute_vertex_program(self.vertex_program)
            memory._iteration = iteration
            for k, v in extra.items():
                memory.set(k, v)
        for mr in ([] if self._map_reduced else self.map_reduces):
            emitted = []
            for vid in (vids if vids is not None else []):
                mr.map(int(vid), props.get(int(vid), {}), lambda k, v: emitted.append((k, v)))
            final = getattr(mr, "generate_final_result", None)
            memory.set(mr.memory_key, final(emitted) if final else iter(emitted))
        result_graph = self._write_back(props)
        memory._runtime = int(round((time.perf_counter() - t0) * 1000))
        return ComputerResult(result_graph, memory)

    def _execute_vertex_program(self, vp):
        g0 = self.graph
        ctx = self._ctx()
        if isinstance(vp, PageRankVertexProgram):
            vid, src, dst, _ = g0.snapshot()
            if vp.max_iterations == 0:
                return vid, {}, 0, {}
            g = ctx.build(vid, src, dst, flags=_lib.ADJ_IN)
            try:
                if self._top_route(vp):
                    # the map-reduces only want the highest ranks: the ranks stay on the device, the longest
                    # list is selected there (jg_pagerank_top) and no per-vertex props are built
                    g.pagerank_begin(vp.damping_factor, vp.vertex_count)
                    g.pagerank_step(vp.max_iterations - 1)
                    tvid, _, trank, _ = g.pagerank_top(max(mr.k for mr in self.map_reduces))
                    top = [(int(v), float(r)) for v, r in zip(tvid, trank)]
                    self._map_reduced = True
                    return vid, {}, vp.max_iterations, {mr.memory_key: top[:mr.k] for mr in self.map_reduces}
                rank, ec = g.pagerank(vp.damping_factor, vp.vertex_count, vp.max_iterations)
            finally:
                g.close()
            props = {int(v): {vp.PAGE_RANK: float(r), vp.OUTGOING_EDGE_COUNT: float(c)}
                     for v, r, c in zip(vid, rank, ec)}
            return vid, props, vp.max_iterations, {}
        if isinstance(vp, ShortestDistanceVertexProgram):
            vid, src, dst, w = g0.snapshot(weight_property=vp.weight_property)
            g = ctx.build(vid, src, dst, weight=w, flags=_lib.ADJ_IN | _lib.ADJ_OUT)
            try:
                dist = g.shortest_distance(vp.seed, vp.max_depth)
            finally:
                g.close()
            props = {int(v): {vp.DISTANCE: int(d)} for v, d in zip(vid, dist) if d != _lib.DIST_ABSENT}
            return vid, props, vp.max_depth, {}
        if isinstance(vp, ConnectedComponentVertexProgram):
            vid, src, dst, _ = g0.snapshot()
            g = self._program_graph(ctx, vid, src, dst, vp.edge_labels, _lib.ADJ_BOTH)
            try:
                if self._census_route(vp) and g.info()["num_shards"] == 1:
                    # the map-reduces only group the labels: the census is made on the device
                    # (jg_cc_census), no label is handed back and no per-vertex props are built
                    it, count, _, cvid, cpop = g.cc_census(1)
                    population = {str(int(c)): int(p) for c, p in zip(cvid, cpop)}
                    self._map_reduced = True
                    return vid, {}, it, {mr.memory_key: count if isinstance(mr, ClusterCountMapReduce)
                                         else dict(population) for mr in self.map_reduces}
                comp, it = g.connected_components()
            finally:
                g.close()
            props = {int(v): {vp.property: str(int(c))} for v, c in zip(vid, comp)}
            return vid, props, it, {}
        if isinstance(vp, PeerPressureVertexProgram):
            vid, src, dst, _ = g0.snapshot()
            direction = PeerPressureVertexProgram.SCOPES[vp.edges]
            g = self._program_graph(ctx, vid, src, dst, vp.edge_labels,
                                    _lib.ADJ_IN if direction == _lib.DIR_OUT else _lib.ADJ_BOTH)
            try:
                if g.info()["num_shards"] != 1:
                    # jg_peer_pressure runs on one shard: the Java side keeps delegating
                    raise ProgramNotSupported("PeerPressureVertexProgram is not run on a sharded graph; "
                                              "delegate to FulgoraGraphComputer")
                cluster, it = g.peer_pressure(direction, vp.distribute_vote, vp.max_iterations)
            finally:
                g.close()
            props = {int(v): {vp.property: int(c)} for v, c in zip(vid, cluster)}  # the Long id, not a String
            return vid, props, it, {}
        if isinstance(vp, ShortestPathVertexProgram):
            return self._shortest_paths(ctx, vp)
        if isinstance(vp, CombinerVertexProgram):
            vid, src, dst, _ = g0.snapshot()
            direction = CombinerVertexProgram.SCOPES[vp.scope]
            adj = {_lib.DIR_OUT: _lib.ADJ_OUT, _lib.DIR_IN: _lib.ADJ_IN, _lib.DIR_BOTH: _lib.ADJ_BOTH}[direction]
            g = self._program_graph(ctx, vid, src, dst, vp.labels, adj)
            try:
                x, received = g.combine_steps(direction, CombinerVertexProgram.COMBINERS.index(vp.combiner), vp.length,
                                              np.full(len(vid), vp.initial_message, np.int64), vp.int32)
            finally:
                g.close()
            # a sum always sets the key (reduce(0, +)); min/max only where a message arrived
            keep = np.ones(len(vid), bool) if vp.combiner == "sum" else received
            props = {int(v): {vp.property_key: int(d)} for v, d, k in zip(vid, x, keep) if k}
            return vid, props, vp.length, {}
        raise ProgramNotSupported(type(vp).__name__)

    def _census_route(self, vp):
        """Whether a ConnectedComponentVertexProgram submission needs the component census only: nothing is
        persisted and every map-reduce is ClusterCountMapReduce / ClusterPopulationMapReduce over the
        program's component property.  (The caller also needs a graph of one shard: jg_cc_census.)"""
        return (self.persist_mode is Persist.NOTHING and bool(self.map_reduces)
                and all(type(mr) in (ClusterCountMapReduce, ClusterPopulationMapReduce)
                        and mr.cluster_property == vp.property for mr in self.map_reduces))

    def _top_route(self, vp):
        """Whether a PageRankVertexProgram submission needs the highest-ranked vertices only: nothing is
        persisted and every map-reduce is a PageRankTopMapReduce (each gets its own prefix of one device
        list, jg_pagerank_top)."""
        return (self.persist_mode is Persist.NOTHING and bool(self.map_reduces)
                and all(type(mr) is PageRankTopMapReduce for mr in self.map_reduces))

    def _edge_scope(self, labels):
        """A label scope over snapshot()'s edge list, worked out once per run: (label id per edge, the scope's label
        ids, one flag per edge: the edge is in the scope); None for labels None (every edge).  A name the graph does
        not know gets an id no edge has, so it matches nothing, as BasicVertexCentricQueryBuilder.java:484 skips
        unknown types."""
        if labels is None:
            return None
        lab, ids = self.graph.edge_label_ids()
        unknown = len(ids)
        scope_ids = [ids.get(name, unknown) for name in labels]
        return lab, scope_ids, np.isin(lab, scope_ids)

    def _scope_weights(self, key, scope, float_weights):
        """snapshot() with the weight column of property `key`, and the flags of the edges the weight checks cover.
        Under a label scope only the scope's edges are read; the others count as edges without the property (their
        values may be anything)."""
        if scope is None:
            vid, src, dst, w = self.graph.snapshot(weight_property=key, float_weights=float_weights)
            return vid, src, dst, w, np.ones(len(w), bool)
        vid, src, dst, _ = self.graph.snapshot()
        absent = float("nan") if float_weights else int(_lib.WEIGHT_ABSENT)
        cast = float if float_weights else int
        w = np.asarray([cast(e.properties[key]) if k and key in e.properties else absent
                        for e, k in zip(self.graph.edges, scope[2].tolist())],
                       dtype=np.float64 if float_weights else np.int32)
        return vid, src, dst, w, scope[2]

    def _label_scoped_graph(self, ctx, vid, src, dst, scope, flags, weight=None, numbered=False):
        """The snapshot through a label-keeping builder, cut down to the labels of `scope` (_edge_scope) on the GPU
        (jg_builder_finish_labels); `weight`: the edges' int32 weights, which travel through the select.
        Returns (graph, pos).  numbered: the builder keeps scope ordinals and `flags` carries ADJ_EDGE_INDEX, so
        the scope's k-th kept edge has ordinal k, and pos[k] (Graph.scope_positions) is its position in
        snapshot()'s edge list: a path's Edge objects are graph.edges[pos[ordinal]], the doubles handed to
        set_weights_f64 are w[pos].  Not numbered: pos is None."""
        lab, scope_ids, _ = scope
        b = ctx.builder()
        try:
            b.keep_labels()
            if numbered:
                b.keep_scope_ordinals()
            b.add_vertices(vid)
            b.add_edges(src, dst, weight=weight, label=lab)
            g = b.finish_labels(scope_ids, flags | (_lib.ADJ_EDGE_INDEX if numbered else 0))
        finally:
            b.close()
        if not numbered:
            return g, None
        try:
            return g, g.scope_positions()
        except BaseException:
            g.close()
            raise

    def _program_graph(self, ctx, vid, src, dst, labels, flags, weight=None):
        """The graph a program runs on: every edge (labels None), or the label scope's edges only."""
        if labels is None:
            return ctx.build(vid, src, dst, weight, flags=flags)
        return self._label_scoped_graph(ctx, vid, src, dst, self._edge_scope(labels), flags, weight)[0]

    def _shortest_paths(self, ctx, vp):
        """ShortestPaths.execute: 64 sources per bit-parallel pass.  On one shard the depth rows stay on the
        device (jg_bfs_keep) and each source's predecessor DAG is built there (jg_bfs_kept_dag): only the DAG
        comes back, and DevicePathDag enumerates it.  Sharded graphs take one depth row per source
        (jg_bfs_rows) and PathDag walks back over the snapshot's BOTH adjacency on the host.  Both routes
        give the same paths in the same order.

        edgeDirection("out" | "in") follows the edges one way: the same two routes with that direction, the
        predecessors read from the reverse adjacency (ADJ_IN | ADJ_OUT is built instead of ADJ_BOTH).
        distanceProperty(key) goes to _weighted_shortest_paths.

        includeEdges(True): the graph is built with ADJ_EDGE_INDEX and the device route takes the edge-listing
        DAG (jg_bfs_kept_dag_edges); a path is [vid, Edge, vid, ..., vid], each Edge the object
        graph.edges[ordinal] (snapshot() lists the edges in that order).  One shard only."""
        if vp.distance_property is not None:
            return self._weighted_shortest_paths(ctx, vp)
        direction = _PATH_DIRECTIONS[vp.edge_direction]
        reverse = _REVERSE_DIRECTION[direction]
        vid, src, dst, _ = self.graph.snapshot()
        sources, target = _path_endpoints(vp, vid)
        both = direction == _lib.DIR_BOTH
        flags = _lib.ADJ_BOTH if both else _lib.ADJ_IN | _lib.ADJ_OUT
        pos = None  # a numbered label scope: the snapshot position of each of its edge ordinals
        try:
            if vp.edge_labels is not None:
                g, pos = self._label_scoped_graph(ctx, vid, src, dst, self._edge_scope(vp.edge_labels), flags,
                                                  numbered=vp.include_edges)
            else:
                g = ctx.build(vid, src, dst, flags=flags | (_lib.ADJ_EDGE_INDEX if vp.include_edges else 0))
        except _lib.JanusGpuError as e:
            if vp.include_edges and e.code == _lib.JG_ERR_UNSUPPORTED:
                # ordinals are kept on one shard only (JG_ADJ_EDGE_INDEX): the Java side keeps delegating
                raise ProgramNotSupported("ShortestPathVertexProgram with includeEdges is not run on a sharded "
                                          "graph; delegate to FulgoraGraphComputer") from e
            raise
        edges = self.graph.edges if pos is None else [self.graph.edges[k] for k in pos.tolist()]
        paths, max_level = [], 0
        max_depth = _int_bound(vp.max_distance)
        try:
            on_device = g.info()["num_shards"] == 1
            neighbors = g.neighbors if both else (lambda rows: g.neighbors(rows, reverse))
            dag = DevicePathDag(len(vid)) if on_device else PathDag(neighbors, len(vid))
            for b0 in range(0, len(sources), SOURCES_PER_BFS):
                batch = sources[b0:b0 + SOURCES_PER_BFS]
                if vp.include_edges:
                    g.bfs_keep(vid[batch], direction, max_depth)
                    for j, s in enumerate(batch):
                        got, deepest = dag.edge_paths(g.bfs_kept_dag_edges(j, target), s, target)
                        max_level = max(max_level, deepest)
                        # even positions hold vertex indices, odd ones edge ordinals
                        paths.extend([edges[x] if i & 1 else int(vid[x]) for i, x in enumerate(p)] for p in got)
                    continue
                if on_device:
                    g.bfs_keep(vid[batch], direction, max_depth)
                    results = (dag.paths(g.bfs_kept_dag(j, target), s, target) for j, s in enumerate(batch))
                else:
                    rows = g.bfs_rows(vid[batch], direction, max_depth)
                    results = (dag.paths(depth, s, target) for s, depth in zip(batch, rows))
                for got, deepest in results:
                    max_level = max(max_level, deepest)
                    paths.extend([int(vid[x]) for x in p] for p in got)
        finally:
            g.close()
        return vid, {}, max_level + 1, {vp.SHORTEST_PATHS: paths}

    def _weighted_shortest_paths(self, ctx, vp):
        """ShortestPathVertexProgram with a distanceProperty: per source, the smallest summed weights stay on
        the device (jg_sssp_keep, delta-stepping along edgeDirection), the tight-edge predecessor DAG to the
        targets within maxDistance (inclusive, on the summed weight) is built there (jg_sssp_kept_dag), and
        DevicePathDag enumerates it: sources in the given order, targets ascending, first predecessor first.
        A float among the edges' values takes _f64_shortest_paths instead (a Double property).
        Refused (the caller delegates): an edge without the property or with a weight < 1 (zero-weight edges
        make the tight-edge graph cyclic; TinkerPop reads any Number), and graphs of several shards.
        The iteration count is 1 + the edges of the longest returned path (1 when there is none): what
        max_level + 1 means on the hop route; this project's rule, not pinned by any reference test."""
        direction = _PATH_DIRECTIONS[vp.edge_direction]
        key = vp.distance_property
        scope = self._edge_scope(vp.edge_labels)
        inside = self.graph.edges if scope is None else [e for e, k in zip(self.graph.edges, scope[2].tolist()) if k]
        if any(isinstance(e.properties.get(key), (float, np.floating)) for e in inside):
            return self._f64_shortest_paths(ctx, vp, scope, inside)
        vid, src, dst, w, checked = self._scope_weights(key, scope, False)
        ws = w[checked]  # the checks cover the scope's edges only
        if len(ws) and int(ws.min()) < 1:
            missing = int((ws == _lib.WEIGHT_ABSENT).sum())
            raise ProgramNotSupported(
                f"ShortestPathVertexProgram with distanceProperty {vp.distance_property!r} is not run by "
                f"GpuGraphComputer: " + (f"{missing} edge(s) lack the property" if missing else
                                         "an edge has a weight < 1") + "; delegate to FulgoraGraphComputer")
        sources, target = _path_endpoints(vp, vid)
        both = direction == _lib.DIR_BOTH
        flags = (_lib.ADJ_BOTH | _lib.ADJ_WEIGHT_BOTH) if both else _lib.ADJ_IN | _lib.ADJ_OUT
        if scope is None:
            g = ctx.build(vid, src, dst, w, flags=flags)
        else:
            g, _ = self._label_scoped_graph(ctx, vid, src, dst, scope, flags, w)
        paths, longest = [], 0
        max_distance = _int_bound(vp.max_distance)
        try:
            if g.info()["num_shards"] != 1:
                raise ProgramNotSupported("ShortestPathVertexProgram with a distanceProperty is not run on a sharded "
                                          "graph; delegate to FulgoraGraphComputer")
            dag = DevicePathDag(len(vid))
            for s in sources:
                g.sssp_keep(vid[s], direction)
                got, _ = dag.paths(g.sssp_kept_dag(target, max_distance), s, target)
                longest = max([longest] + [len(p) - 1 for p in got])
                paths.extend([int(vid[x]) for x in p] for p in got)
        finally:
            g.close()
        return vid, {}, longest + 1, {vp.SHORTEST_PATHS: paths}

    def _f64_shortest_paths(self, ctx, vp, scope, inside):
        """_weighted_shortest_paths when an edge's value for the key is a float (a Double property): a path's
        length is the IEEE binary64 sum of its weights, ties are exact (jg_graph_set_weights_f64,
        jg_sssp_keep_f64, jg_sssp_kept_dag_f64).  Every value must be a Python / numpy int (converted exactly;
        refused beyond 2^53) or a float64.  Refused (the caller delegates): a missing property, a value of another
        type (a binary32 Float among them: TinkerPop sums those in float arithmetic), a non-finite or <= 0 value,
        weights whose range could absorb a relaxation (the library's JG_ERR_UNSUPPORTED), graphs of several
        shards.  Path order and the iteration rule are _weighted_shortest_paths'."""
        key = vp.distance_property

        def refuse(why):
            return ProgramNotSupported(f"ShortestPathVertexProgram with distanceProperty {key!r} is not run by "
                                       f"GpuGraphComputer: {why}; delegate to FulgoraGraphComputer")

        for e in inside:  # the edges of the label scope `scope` (_edge_scope): the checks cover them only
            x = e.properties.get(key)
            if x is None:
                raise refuse("an edge lacks the property")
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.float64)):
                raise refuse(f"a value of type {type(x).__name__}")
            if isinstance(x, (int, np.integer)) and abs(int(x)) > 2**53:
                raise refuse("an integer beyond 2^53 has no exact double")
        direction = _PATH_DIRECTIONS[vp.edge_direction]
        vid, src, dst, w, checked = self._scope_weights(key, scope, True)
        ws = w[checked]
        if len(ws) and not (np.isfinite(ws).all() and ws.min() > 0):
            raise refuse("a weight is not finite and > 0")
        sources, target = _path_endpoints(vp, vid)
        both = direction == _lib.DIR_BOTH
        flags = _lib.ADJ_BOTH if both else _lib.ADJ_IN | _lib.ADJ_OUT
        try:
            if scope is not None:  # the scope's doubles, in its ordinals' order
                g, pos = self._label_scoped_graph(ctx, vid, src, dst, scope, flags, numbered=True)
                w = w[pos]
            else:
                g = ctx.build(vid, src, dst, flags=flags | _lib.ADJ_EDGE_INDEX)
        except _lib.JanusGpuError as e:
            if e.code == _lib.JG_ERR_UNSUPPORTED:  # edge ordinals are kept on one shard only
                raise refuse("the graph is sharded") from e
            raise
        paths, longest = [], 0
        max_distance = -1.0 if vp.max_distance is None else float(vp.max_distance)
        try:
            try:
                g.set_weights_f64(w)
            except _lib.JanusGpuError as e:
                if e.code == _lib.JG_ERR_UNSUPPORTED:
                    raise refuse("the weights' range could absorb a relaxation") from e
                raise
            dag = DevicePathDag(len(vid))
            for s in sources:
                g.sssp_keep_f64(vid[s], direction)
                got, _ = dag.paths(g.sssp_kept_dag_f64(target, max_distance), s, target)
                longest = max([longest] + [len(p) - 1 for p in got])
                paths.extend([int(vid[x]) for x in p] for p in got)
        finally:
            g.close()
        return vid, {}, longest + 1, {vp.SHORTEST_PATHS: paths}

    def _write_back(self, props):
        if self.persist_mode is Persist.NOTHING:
            return None if self.result_graph_mode is ResultGraph.NEW else self.graph
        if self.result_graph_mode is ResultGraph.ORIGINAL:
            for vid, kv in props.items():
                v = self.graph.vertices.get(vid)
                if v is not None:
                    v.properties.update(kv)
            return self.graph
        return ComputedGraph(self.graph, props)


def _path_endpoints(vp, vid):
    """ShortestPathVertexProgram's sources as snapshot indices (every vertex when none are given; unknown ids are
    skipped) and its targets as one flag per vertex (None: every vertex)."""
    index = {int(v): i for i, v in enumerate(vid.tolist())}
    sources = [index[s] for s in (vp.sources if vp.sources is not None else vid.tolist()) if s in index]
    target = None
    if vp.targets is not None:
        target = np.zeros(len(vid), bool)
        target[[index[t] for t in vp.targets if t in index]] = True
    return sources, target


def _int_bound(d):
    """maxDistance for the hop route and the integer weights' route: int(), -1 (none) for None, inf and NaN."""
    if d is None or (isinstance(d, float) and not np.isfinite(d)):
        return -1
    return int(d)


SOURCES_PER_BFS = 64  # jg_bfs_rows: one bit-parallel pass per 64 sources
_PATH_DIRECTIONS = {"out": _lib.DIR_OUT, "in": _lib.DIR_IN, "both": _lib.DIR_BOTH}  # edgeDirection
_REVERSE_DIRECTION = {_lib.DIR_OUT: _lib.DIR_IN, _lib.DIR_IN: _lib.DIR_OUT, _lib.DIR_BOTH: _lib.DIR_BOTH}


class PathDag:
    """Every shortest path from one source to the targets it reaches, rebuilt from its depth row (mirror
    of GpuGraphComputer.PathDag, java/.../GpuGraphComputer.java): the predecessors of a vertex at depth d
    are its BOTH neighbours at depth d - 1, read level by level from the device snapshot
    (jg_graph_neighbors), deepest targets first, so each vertex on some path is expanded once; paths are
    then enumerated from each target (ascending) back to the source.  `neighbors(rows)` -> (off, nbr)."""

    ROWS_PER_CALL = 1 << 14

    def __init__(self, neighbors, n):
        self.neighbors = neighbors
        self.n = n

    def predecessors(self, depth, target=None):
        """{vertex: predecessor array} for every vertex on a shortest path to a target; and the targets."""
        depth = np.asarray(depth)
        reached = depth >= 0
        if target is not None:
            reached &= target
        targets = np.flatnonzero(reached)
        if len(targets) == 0:
            return {}, targets, -1
        deepest = int(depth[targets].max())
        level = [[] for _ in range(deepest + 1)]
        for d in range(deepest + 1):
            level[d] = list(targets[depth[targets] == d])
        queued = np.zeros(self.n, bool)
        queued[targets] = True
        pred = {}
        for d in range(deepest, 0, -1):
            cur = np.asarray(level[d], np.int64)
            for f in range(0, len(cur), self.ROWS_PER_CALL):
                rows = cur[f:f + self.ROWS_PER_CALL]
                off, nbr = self.neighbors(rows)
                for i, v in enumerate(rows.tolist()):
                    nb = nbr[off[i]:off[i + 1]]
                    nb = nb[depth[nb] == d - 1]
                    _, first = np.unique(nb, return_index=True)
                    p = nb[np.sort(first)]  # distinct, in adjacency order
                    pred[v] = p
                    new = p[~queued[p]]
                    queued[new] = True
                    level[d - 1].extend(new.tolist())
        return pred, targets, deepest

    def paths(self, depth, s, target=None):
        """(paths as vertex-index lists, deepest target depth (0 if none))."""
        pred, targets, deepest = self.predecessors(depth, target)
        out = []
        for t in targets.tolist():
            stack = [(t, [t])]
            while stack:
                v, suffix = stack.pop()
                if v == s:
                    out.append(list(reversed(suffix)))
                    continue
                for u in reversed(pred[v].tolist()):  # first predecessor first, as the Java recursion
                    stack.append((u, suffix + [u]))
        return out, max(deepest, 0)


class DevicePathDag:
    """PathDag.paths' result from a predecessor DAG built on the device (Graph.bfs_kept_dag):
    dag = (vertex, depth, off, pred), vertex[j] with the predecessors pred[off[j]:off[j + 1]], depth
    non-increasing.  Paths are enumerated as PathDag does: targets ascending, first predecessor first.
    The weighted DAG (Graph.sssp_kept_dag) has distances in the depth's place: the enumeration reads only
    the first of them, for the second value it returns (the largest depth / distance of a target)."""

    def __init__(self, n):
        self.n = n

    def paths(self, dag, s, target=None):
        """(paths as vertex-index lists, deepest target depth (0 if none))."""
        vertex, depth, off, pred = dag
        if len(vertex) == 0:
            return [], 0
        pos = np.full(self.n, -1, np.int64)
        pos[vertex] = np.arange(len(vertex))
        targets = np.sort(vertex if target is None else vertex[np.asarray(target, bool)[vertex]])
        off = np.asarray(off).tolist()
        out = []
        for t in targets.tolist():
            stack = [(t, [t])]
            while stack:
                v, suffix = stack.pop()
                if v == s:
                    out.append(list(reversed(suffix)))
                    continue
                j = pos[v]
                for u in reversed(pred[off[j]:off[j + 1]].tolist()):
                    stack.append((u, suffix + [u]))
        return out, int(depth[0])

    def edge_paths(self, dag, s, target=None):
        """`paths` over an edge-listing DAG (Graph.bfs_kept_dag_edges): dag = (vertex, depth, off, pred, edge),
        each path as alternating vertex index and edge ordinal [v, e, v, ..., v] ([s] from s to itself):
        targets ascending, first entry first."""
        vertex, depth, off, pred, edge = dag
        if len(vertex) == 0:
            return [], 0
        pos = np.full(self.n, -1, np.int64)
        pos[vertex] = np.arange(len(vertex))
        targets = np.sort(vertex if target is None else vertex[np.asarray(target, bool)[vertex]])
        off = np.asarray(off).tolist()
        out = []
        for t in targets.tolist():
            stack = [(t, [t])]
            while stack:
                v, suffix = stack.pop()
                if v == s:
                    out.append(list(reversed(suffix)))
                    continue
                j = pos[v]
                b, e = off[j], off[j + 1]
                for u, x in zip(reversed(pred[b:e].tolist()), reversed(edge[b:e].tolist())):
                    stack.append((u, suffix + [x, u]))
        return out, int(depth[0])
