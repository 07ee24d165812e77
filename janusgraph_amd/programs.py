"""Vertex programs and map-reduces that GpuGraphComputer recognises and runs on the GPU.

Same names, configuration keys, builders and output keys as the reference:
  PageRankVertexProgram / PageRankMapReduce
      janusgraph-backend-testutils/src/main/java/org/janusgraph/olap/PageRankVertexProgram.java:46-166,
      PageRankMapReduce.java:32-67
  ShortestDistanceVertexProgram / ShortestDistanceMapReduce
      janusgraph-backend-testutils/.../olap/ShortestDistanceVertexProgram.java:40-192,
      ShortestDistanceMapReduce.java:29-64
  ConnectedComponentVertexProgram, ShortestPathVertexProgram
      TinkerPop 3.4.6 gremlin-core (third party, not in the container; SURVEY.md A.3/A.4 [TP-recall])
  CombinerVertexProgram / DegreeCounter / DegreeMapper
      a superstep loop with a sum / min / max MessageCombiner over one Local scope, as
      janusgraph-test/src/main/java/org/janusgraph/olap/OLAPTest.java:424-540 (DegreeCounter,
      DegreeMapper) writes it; message combining per VertexState.java:85-114
Any other program is not recognised: the computer refuses it with ProgramNotSupported so that the
caller (the Java GpuGraphComputer) delegates it to FulgoraGraphComputer unchanged.
"""
from __future__ import annotations

from .computer_types import Persist, ResultGraph


class VertexProgram:
    """Configuration-carrying program (storeState/loadState as a dict)."""

    VERTEX_PROGRAM = "gremlin.vertexProgram"
    preferred_result_graph = ResultGraph.ORIGINAL
    preferred_persist = Persist.VERTEX_PROPERTIES
    compute_keys: tuple = ()

    def __init__(self, configuration: dict):
        self.configuration = dict(configuration)
        self.load_state(self.configuration)

    def load_state(self, conf):
        pass

    def store_state(self) -> dict:
        return dict(self.configuration, **{self.VERTEX_PROGRAM: type(self).__name__})

    def get_map_reducers(self):
        return []


EDGE_LABELS = "edgeLabels"  # configuration key of the label-scoped programs (a tuple of label names, or None)


def _edge_labels(labels):
    """The `edgeLabels` configuration value as a tuple of label names (None: every edge): a program's edges named
    by label, the bothE("knows") of ShortestPath.edges / ConnectedComponent.edges / PeerPressure's by().  As
    CombinerVertexProgram.labels: at least one name, every name a string; an empty name is refused too."""
    if labels is None:
        return None
    if isinstance(labels, str):
        labels = (labels,)
    try:
        labels = tuple(labels)
    except TypeError:
        raise ValueError("edgeLabels must name at least one edge label") from None
    if not labels or not all(isinstance(x, str) and x for x in labels):
        raise ValueError("edgeLabels must name at least one edge label, each a non-empty string")
    return labels


class _Builder:
    def __init__(self, cls):
        self.cls = cls
        self.configuration = {}

    def create(self, graph=None):
        return self.cls(self.configuration)


class _LabelScopedBuilder(_Builder):
    """The builder of a program whose edges may be named by label (the `edgeLabels` key)."""

    def edgeLabels(self, *names):  # noqa: N802
        self.configuration[EDGE_LABELS] = _edge_labels(names)
        return self


class PageRankVertexProgram(VertexProgram):
    PAGE_RANK = "janusgraph.pageRank.pageRank"
    OUTGOING_EDGE_COUNT = "janusgraph.pageRank.edgeCount"
    DAMPING_FACTOR = "janusgraph.pageRank.dampingFactor"
    MAX_ITERATIONS = "janusgraph.pageRank.maxIterations"
    VERTEX_COUNT = "janusgraph.pageRank.vertexCount"
    compute_keys = (PAGE_RANK, OUTGOING_EDGE_COUNT)

    def load_state(self, conf):  # PageRankVertexProgram.java:64-69
        self.damping_factor = float(conf.get(self.DAMPING_FACTOR, 0.85))
        self.max_iterations = int(conf.get(self.MAX_ITERATIONS, 10))
        self.vertex_count = int(conf.get(self.VERTEX_COUNT, 1))

    class Builder(_Builder):
        def __init__(self):
            super().__init__(PageRankVertexProgram)

        def vertexCount(self, n):  # noqa: N802 (reference names)
            self.configuration[PageRankVertexProgram.VERTEX_COUNT] = int(n)
            return self

        def dampingFactor(self, d):  # noqa: N802
            self.configuration[PageRankVertexProgram.DAMPING_FACTOR] = float(d)
            return self

        def iterations(self, k):
            self.configuration[PageRankVertexProgram.MAX_ITERATIONS] = int(k)
            return self

    @classmethod
    def build(cls):
        return cls.Builder()


class ShortestDistanceVertexProgram(VertexProgram):
    DISTANCE = "janusgraph.shortestDistanceVertexProgram.distance"
    MAX_DEPTH = "janusgraph.shortestDistanceVertexProgram.maxDepth"
    WEIGHT_PROPERTY = "janusgraph.shortestDistanceVertexProgram.weightProperty"
    SEED = "janusgraph.shortestDistanceVertexProgram.seedID"
    compute_keys = (DISTANCE,)

    def load_state(self, conf):  # ShortestDistanceVertexProgram.java:65-71
        if self.MAX_DEPTH not in conf or self.SEED not in conf:
            raise KeyError("maxDepth and seed are required")
        self.max_depth = int(conf[self.MAX_DEPTH])
        self.seed = int(conf[self.SEED])
        self.weight_property = conf.get(self.WEIGHT_PROPERTY, "distance")

    class Builder(_Builder):
        def __init__(self):
            super().__init__(ShortestDistanceVertexProgram)

        def maxDepth(self, d):  # noqa: N802
            self.configuration[ShortestDistanceVertexProgram.MAX_DEPTH] = int(d)
            return self

        def seed(self, vid):
            self.configuration[ShortestDistanceVertexProgram.SEED] = int(vid)
            return self

        def weightProperty(self, key):  # noqa: N802
            self.configuration[ShortestDistanceVertexProgram.WEIGHT_PROPERTY] = key
            return self

    @classmethod
    def build(cls):
        return cls.Builder()


class ConnectedComponentVertexProgram(VertexProgram):
    COMPONENT = "gremlin.connectedComponentVertexProgram.component"
    PROPERTY = "gremlin.connectedComponentVertexProgram.property"
    MAX_ITERATIONS = "gremlin.connectedComponentVertexProgram.maxIterations"
    compute_keys = (COMPONENT,)

    def load_state(self, conf):
        self.property = conf.get(self.PROPERTY, self.COMPONENT)
        self.max_iterations = int(conf.get(self.MAX_ITERATIONS, 100))
        if self.max_iterations != 100:
            raise ValueError("GpuGraphComputer runs ConnectedComponentVertexProgram with maxIterations = 100")
        # edgeLabels (None: every edge): connectedComponent().with(ConnectedComponent.edges, bothE("knows")); only
        # edges of those labels join vertices, a name the graph does not know matches nothing
        self.edge_labels = _edge_labels(conf.get(EDGE_LABELS))

    class Builder(_LabelScopedBuilder):
        def __init__(self):
            super().__init__(ConnectedComponentVertexProgram)

        def property(self, key):
            self.configuration[ConnectedComponentVertexProgram.PROPERTY] = key
            return self

    @classmethod
    def build(cls):
        return cls.Builder()


class ShortestPathVertexProgram(VertexProgram):
    """Depth on the GPU (Fulgora forces {Local(bothE), Global}), paths rebuilt on the host.

    TinkerPop's two further knobs [TP-recall]: distanceProperty(key) makes a path's length the sum of that edge
    property (Integer >= 1, or Double: finite and > 0, summed in IEEE binary64 with exact ties only; anything
    else is refused with ProgramNotSupported at submit), and maxDistance then bounds that sum, inclusive; edgeDirection("out" | "in" | "both") restricts the edges a path follows
    (default "both").  memory.getIteration() is 1 + the number of edges of the longest returned path (1 when
    there is none), with or without a distance property: this project's rule, not pinned by any reference
    test.

    includeEdges(True) returns each path as [vid, Edge, vid, ..., vid], the Edge objects being the graph's own:
    two parallel edges between the same vertices give two paths.  It runs on the hop route only; together
    with a distanceProperty it is refused (ValueError).

    edgeLabels("knows", ...) (the `edgeLabels` key; None: every edge) names the edges a path may follow, the
    bothE("knows") of ShortestPath.edges: honoured on every route, and the weight checks of a distanceProperty
    then cover the named edges only.  A name the graph does not know matches nothing."""

    SHORTEST_PATHS = "gremlin.shortestPathVertexProgram.shortestPaths"
    EDGE_DIRECTIONS = ("out", "in", "both")
    preferred_persist = Persist.NOTHING

    def load_state(self, conf):
        self.sources = conf.get("sources")  # None = every vertex
        self.targets = conf.get("targets")  # None = every vertex
        self.max_distance = conf.get("maxDistance")
        self.include_edges = bool(conf.get("includeEdges", False))
        self.distance_property = conf.get("distanceProperty")
        if self.include_edges and self.distance_property is not None:
            raise ValueError("includeEdges together with a distanceProperty is not supported by GpuGraphComputer")
        if self.distance_property is not None and (not isinstance(self.distance_property, str)
                                                   or not self.distance_property):
            raise ValueError("distanceProperty must name an edge property")
        self.edge_direction = conf.get("edgeDirection", "both")
        if self.edge_direction not in self.EDGE_DIRECTIONS:
            raise ValueError('edgeDirection must be "out", "in" or "both"')
        self.edge_labels = _edge_labels(conf.get(EDGE_LABELS))

    class Builder(_LabelScopedBuilder):
        def __init__(self):
            super().__init__(ShortestPathVertexProgram)

        def source(self, *vids):
            self.configuration["sources"] = [int(v) for v in vids]
            return self

        def target(self, *vids):
            self.configuration["targets"] = [int(v) for v in vids]
            return self

        def maxDistance(self, d):  # noqa: N802
            # a non-integral bound is kept (the sums of a Double distanceProperty); the hop route and the integer
            # weights' route apply int() to it
            self.configuration["maxDistance"] = int(d) if float(d).is_integer() else float(d)
            return self

        def includeEdges(self, include):  # noqa: N802
            self.configuration["includeEdges"] = bool(include)
            return self

        def distanceProperty(self, key):  # noqa: N802
            if not isinstance(key, str) or not key:
                raise ValueError("distanceProperty must name an edge property")
            self.configuration["distanceProperty"] = key
            return self

        def edgeDirection(self, d):  # noqa: N802
            d = d.lower() if isinstance(d, str) else d
            if d not in ShortestPathVertexProgram.EDGE_DIRECTIONS:
                raise ValueError('edgeDirection must be "out", "in" or "both"')
            self.configuration["edgeDirection"] = d
            return self

    @classmethod
    def build(cls):
        return cls.Builder()


class CombinerVertexProgram(VertexProgram):
    """A program whose every superstep is x_t[v] = COMBINE of the messages v receives, each neighbour
    sending its x_{t-1}: superstep 0 sends `initial_message`, supersteps 1..length store the combined
    value under `property_key` and send it on while t < length; terminate at iteration >= length.
    `scope` is the send scope's direction: "inE" (DegreeCounter's DEG_MSG, OLAPTest.java:429) reaches
    the sources of a vertex's in-edges, so a vertex receives from its out-neighbours.
    `labels` (a tuple of edge label names, None: every edge) types the scope, the __.inE("a", "b") of
    MessageScope.Local: only edges of those labels carry messages (one fitted slice per label,
    BasicVertexCentricQueryBuilder.java:482-587); a name the graph does not know matches nothing."""

    preferred_result_graph = ResultGraph.NEW
    preferred_persist = Persist.VERTEX_PROPERTIES
    COMBINERS = ("sum", "min", "max")
    SCOPES = {"inE": 1, "outE": 2, "bothE": 3}  # -> the receiver's pull direction (DIR_OUT/IN/BOTH)

    def __init__(self, length=1, property_key="degree", combiner="sum", scope="inE", initial_message=1,
                 int32=True, labels=None):
        if length <= 0:
            raise ValueError("length must be positive")  # Preconditions.checkArgument(length>0), :438
        if combiner not in self.COMBINERS or scope not in self.SCOPES:
            raise ValueError("unknown combiner or scope")
        self.length, self.property_key, self.combiner, self.scope = length, property_key, combiner, scope
        self.initial_message, self.int32 = initial_message, int32
        if labels is not None:
            if isinstance(labels, str):
                labels = (labels,)
            labels = tuple(labels)
            if not labels or not all(isinstance(x, str) for x in labels):
                raise ValueError("labels must name at least one edge label")
        self.labels = labels
        self.compute_keys = (property_key,)
        super().__init__({"length": length})


class DegreeCounter(CombinerVertexProgram):
    """OLAPTest.DegreeCounter (OLAPTest.java:424-503): k-hop out-path counts, Integer sums."""

    DEGREE = "degree"

    def __init__(self, length=1):
        super().__init__(length, self.DEGREE, "sum", "inE", 1, True)


class MapReduce:
    memory_key = None

    def map(self, vid, props, emit):
        raise NotImplementedError


class PageRankMapReduce(MapReduce):
    DEFAULT_MEMORY_KEY = "pageRank"

    def __init__(self, memory_key=DEFAULT_MEMORY_KEY):
        self.memory_key = memory_key

    @classmethod
    def build(cls):
        return _MrBuilder(cls)

    def map(self, vid, props, emit):  # PageRankMapReduce.java:62-67
        v = props.get(PageRankVertexProgram.PAGE_RANK)
        if v is not None:
            emit(vid, v)


class ShortestDistanceMapReduce(MapReduce):
    DEFAULT_MEMORY_KEY = "shortestDistance"

    def __init__(self, memory_key=DEFAULT_MEMORY_KEY):
        self.memory_key = memory_key

    @classmethod
    def build(cls):
        return _MrBuilder(cls)

    def map(self, vid, props, emit):  # ShortestDistanceMapReduce.java:59-64
        v = props.get(ShortestDistanceVertexProgram.DISTANCE)
        if v is not None:
            emit(vid, v)


class DegreeMapper(MapReduce):
    """OLAPTest.DegreeMapper (OLAPTest.java:505-540): memory["degrees"] = {vertex id: degree}."""

    DEGREE_RESULT = "degrees"
    memory_key = DEGREE_RESULT

    def map(self, vid, props, emit):
        v = props.get(DegreeCounter.DEGREE)
        if v is not None:
            emit(vid, v)

    def generate_final_result(self, key_values):
        return {k: v for k, v in key_values}


class _MrBuilder:
    def __init__(self, cls):
        self.cls, self.key = cls, cls.DEFAULT_MEMORY_KEY

    def memoryKey(self, key):  # noqa: N802
        self.key = key
        return self

    def create(self):
        return self.cls(self.key)


class _TopMrBuilder(_MrBuilder):
    def __init__(self, cls):
        super().__init__(cls)
        self.k = 10

    def limit(self, k):
        self.k = int(k)
        return self

    def create(self):
        return self.cls(self.k, self.key)


class PageRankTopMapReduce(MapReduce):
    """The k highest-ranked vertices of a PageRankVertexProgram run: memory[memory_key] = a list of (vertex id,
    rank), rank descending by numeric value (-0.0 as +0.0, NaN last), ties in emission order, which is the
    snapshot's vertex order.  This project's own class, not one of the reference's: it is what a
    PageRankMapReduce emission followed by an ordering on the caller's side boils down to.  After
    PageRankVertexProgram, with Persist.NOTHING and no other kind of map-reduce, GpuGraphComputer takes the
    list from the device select (jg_pagerank_top) instead of this map."""

    DEFAULT_MEMORY_KEY = "pageRankTop"

    def __init__(self, k, memory_key=DEFAULT_MEMORY_KEY):
        if int(k) < 1:
            raise ValueError(f"k must be at least 1: {k}")
        self.k = int(k)
        self.memory_key = memory_key

    @classmethod
    def build(cls):
        return _TopMrBuilder(cls)

    def map(self, vid, props, emit):  # as PageRankMapReduce.map
        v = props.get(PageRankVertexProgram.PAGE_RANK)
        if v is not None:
            emit(vid, v)

    def generate_final_result(self, key_values):
        def order(kv):
            r = kv[1]
            return (1, 0.0) if r != r else (0, -(r + 0.0))
        return sorted(key_values, key=order)[:self.k]  # stable: ties keep emission order


# TinkerPop's PeerPressureVertexProgram.CLUSTER, the property the cluster map-reduces read by default
PEER_PRESSURE_CLUSTER = "gremlin.peerPressureVertexProgram.cluster"


class PeerPressureVertexProgram(VertexProgram):
    """TinkerPop 3.4.6 PeerPressureVertexProgram (third party, not in the container; [TP-recall]): every
    vertex starts in its own cluster and joins, superstep after superstep, the cluster with the largest summed
    vote strength among its own vote and the votes it receives; with distributeVote a vertex's strength is
    1 / (edges it votes along).  Votes travel along `edges` ("outE", the default, or "bothE").  The stored
    cluster is the Long id of a vertex.  Among exactly tied clusters GpuGraphComputer takes the numerically
    smallest id (TinkerPop's choice follows HashMap order and is not defined).  edgeLabels("knows", ...) (the
    `edgeLabels` key; None: every edge) names the edges votes travel along, as peerPressure().by(outE("knows"))."""

    CLUSTER = PEER_PRESSURE_CLUSTER
    VOTE_STRENGTH = "gremlin.peerPressureVertexProgram.voteStrength"
    PROPERTY = "gremlin.peerPressureVertexProgram.property"
    MAX_ITERATIONS = "gremlin.peerPressureVertexProgram.maxIterations"
    DISTRIBUTE_VOTE = "gremlin.peerPressureVertexProgram.distributeVote"
    EDGES = "gremlin.peerPressureVertexProgram.edgeTraversal"
    SCOPES = {"outE": 1, "bothE": 3}  # -> jg_peer_pressure's direction (DIR_OUT / DIR_BOTH)
    preferred_result_graph = ResultGraph.NEW
    preferred_persist = Persist.VERTEX_PROPERTIES
    compute_keys = (CLUSTER, VOTE_STRENGTH)

    def load_state(self, conf):
        self.property = conf.get(self.PROPERTY, self.CLUSTER)
        self.max_iterations = int(conf.get(self.MAX_ITERATIONS, 30))
        self.distribute_vote = bool(conf.get(self.DISTRIBUTE_VOTE, False))
        self.edges = conf.get(self.EDGES, "outE")
        if self.max_iterations < 0:
            raise ValueError("maxIterations must not be negative")
        if self.edges not in self.SCOPES:
            raise ValueError(f"GpuGraphComputer runs PeerPressureVertexProgram over outE or bothE, not {self.edges!r}")
        self.compute_keys = (self.property, self.VOTE_STRENGTH)
        self.edge_labels = _edge_labels(conf.get(EDGE_LABELS))

    class Builder(_LabelScopedBuilder):
        def __init__(self):
            super().__init__(PeerPressureVertexProgram)

        def property(self, key):
            self.configuration[PeerPressureVertexProgram.PROPERTY] = key
            return self

        def maxIterations(self, k):  # noqa: N802
            self.configuration[PeerPressureVertexProgram.MAX_ITERATIONS] = int(k)
            return self

        def distributeVote(self, on):  # noqa: N802
            self.configuration[PeerPressureVertexProgram.DISTRIBUTE_VOTE] = bool(on)
            return self

        def edges(self, scope):
            if scope not in PeerPressureVertexProgram.SCOPES:
                raise ValueError(f"edges must be 'outE' or 'bothE', not {scope!r}")
            self.configuration[PeerPressureVertexProgram.EDGES] = scope
            return self

    @classmethod
    def build(cls):
        return cls.Builder()


class _ClusterMrBuilder(_MrBuilder):
    def __init__(self, cls):
        super().__init__(cls)
        self.cluster = PEER_PRESSURE_CLUSTER

    def clusterProperty(self, key):  # noqa: N802
        self.cluster = key
        return self

    def create(self):
        return self.cls(self.key, self.cluster)


class ClusterCountMapReduce(MapReduce):
    """TinkerPop 3.4.6 ClusterCountMapReduce (third party, not in the container; [TP-recall]): every vertex
    that has the cluster property emits it under one null key, the final result is the number of distinct
    clusters (an int).  Default memory key "clusterCount"; the cluster property defaults to
    PeerPressureVertexProgram.CLUSTER and is configurable (clusterProperty), e.g. to
    ConnectedComponentVertexProgram's component key.  After that program, with Persist.NOTHING on one
    shard, GpuGraphComputer takes the result from the device census (jg_cc_census) instead of this map."""

    DEFAULT_MEMORY_KEY = "clusterCount"

    def __init__(self, memory_key=DEFAULT_MEMORY_KEY, cluster_property=PEER_PRESSURE_CLUSTER):
        self.memory_key = memory_key
        self.cluster_property = cluster_property

    @classmethod
    def build(cls):
        return _ClusterMrBuilder(cls)

    def map(self, vid, props, emit):
        c = props.get(self.cluster_property)
        if c is not None:
            emit(None, c)

    def generate_final_result(self, key_values):
        return len({v for _, v in key_values})


class ClusterPopulationMapReduce(MapReduce):
    """TinkerPop 3.4.6 ClusterPopulationMapReduce ([TP-recall], as above): every vertex that has the cluster
    property emits (cluster, 1), the counts are summed per cluster, the final result is a dict cluster ->
    population whose keys are the values the program stored (for ConnectedComponentVertexProgram: the label
    Strings).  Default memory key "clusterPopulation"; cluster property as for ClusterCountMapReduce."""

    DEFAULT_MEMORY_KEY = "clusterPopulation"

    def __init__(self, memory_key=DEFAULT_MEMORY_KEY, cluster_property=PEER_PRESSURE_CLUSTER):
        self.memory_key = memory_key
        self.cluster_property = cluster_property

    @classmethod
    def build(cls):
        return _ClusterMrBuilder(cls)

    def map(self, vid, props, emit):
        c = props.get(self.cluster_property)
        if c is not None:
            emit(c, 1)

    def generate_final_result(self, key_values):
        out = {}
        for k, v in key_values:
            out[k] = out.get(k, 0) + v
        return out


RECOGNISED = (PageRankVertexProgram, ShortestDistanceVertexProgram, ConnectedComponentVertexProgram,
              ShortestPathVertexProgram, CombinerVertexProgram, PeerPressureVertexProgram)
