"""Edgestore rows whose every edge has a relation id of its own, with the edge list they hold known by
construction (the fixtures of tests/test_row_edges_host.py and tests/test_gpu_row_edges.py).

A rows builder that keeps relation ids numbers the decoder's kept list: every visible OUT user edge on a
processed row (a live vertex's own row, or a non-canonical representative of a vertex-cut vertex), in row
(key) order then entry (column) order, ghost-ended edges included.  RowStore records, for every entry it
writes, whether it is such an entry and which relation it holds, so `listed()` is that list without any
decoder: (src, dst, relation id, entry index) per listed edge.
"""
import struct

import numpy as np

from janusgraph_amd.idmanager import IDManager
from oracle import edgecodec as ec

VERTEX_EXISTS = ec.schema_id(1, "system_key")
NAME_KEY = ec.schema_id(5, "user_key")      # a vertex property (a row entry, not an edge property)
LABELS = [ec.schema_id(c, "user_edge") for c in (11, 12, 13, 14)]
MULTS = [ec.MULTI, ec.SIMPLE, ec.ONE2MANY, ec.MANY2ONE]
TIDS = np.array(LABELS[1:], np.int64)
TMULT = np.array(MULTS[1:], np.int8)
SYS_EDGE = ec.schema_id(2, "system_edge")

# edge properties, ascending key ids: a Long and a String in front of the weight key
LONG_KEY = ec.schema_id(6, "user_key")
STR_KEY = ec.schema_id(7, "user_key")
W_KEY = ec.schema_id(9, "user_key")
CHUNK = 1024  # kChunk of jg_decode.hip: entries per block iteration of edgestore_edges_kernel


def key_table(wtype):
    """(weight key inline id, key inline ids, key types) for set_weight_key / set_weight_key_f64."""
    keys = {LONG_KEY: ec.LONG, STR_KEY: ec.STRING, W_KEY: wtype}
    return ec.inline_id(W_KEY), [ec.inline_id(k) for k in keys], list(keys.values())


def enc_double(x):
    """DoubleSerializer.write: putDouble, the big-endian IEEE bits."""
    return struct.pack(">d", x)


def enc_long(v):
    """LongSerializer.write: value - Long.MIN_VALUE as 8 big-endian bytes (the sign bit flipped)."""
    return ((int(v) + (1 << 63)) & ((1 << 64) - 1)).to_bytes(8, "big")


def weight_value(wtype, w, rng=None, pad=None):
    """An edge value holding the weight `w` under W_KEY as type `wtype` (None: no weight property; "null": a
    null value).  pad: the length of the String property in front of it (with a Long before that), else a
    random choice of the two."""
    props = []
    if pad is not None or (rng is not None and rng.random() < 0.5):
        props.append((LONG_KEY, ec.LONG, enc_long(int(rng.integers(-(1 << 40), 1 << 40)) if rng is not None else 7)))
    if pad is not None:
        props.append((STR_KEY, ec.STRING, "abcdefghi"[:pad]))
    elif rng is not None and rng.random() < 0.5:
        props.append((STR_KEY, ec.STRING, [None, "", "x", "abc" * 5, "é"][int(rng.integers(0, 5))]))
    if w is not None:
        if w == "null":
            props.append((W_KEY, wtype, None))
        elif wtype == ec.DOUBLE:
            props.append((W_KEY, wtype, enc_double(w)))
        elif wtype == ec.LONG:
            props.append((W_KEY, wtype, enc_long(w)))
        else:
            props.append((W_KEY, wtype, int(w)))
    return ec.write_properties(props)


class RowStore:
    def __init__(self, pbits=5):
        self.pbits = pbits
        self.idm = IDManager(pbits)
        self.rows = {}     # row vertex id -> [(entry bytes, value position, relation id of an OUT user edge or -1)]
        self.live = set()  # canonical ids whose row starts with VertexExists
        self.ends = {}     # relation id -> (canonical source, canonical target)
        self.edge_no = {}  # store_random: relation id -> the edge's number e (what value_of was called with)
        self.rel = 1000

    def vid(self, count, partition=0, suffix=0):
        return (((count << self.pbits) + partition) << 3) | suffix

    def canon(self, v):
        from oracle.oracle import canonical_vertex_id
        if v & 7 == 2 and self.pbits > 0 and v >> (self.pbits + 3) > 0:
            return canonical_vertex_id(v, self.pbits)
        return v

    def next_rel(self):
        self.rel += 1
        return self.rel

    def vertex(self, v, live=True):
        self.rows.setdefault(v, [])
        if live:
            self.rows[v].append(ec.encode_property(VERTEX_EXISTS, self.next_rel(), b"\x01") + (-1,))
            self.live.add(v)
        return v

    def prop(self, v, value=b"x"):
        self.rows.setdefault(v, []).append(ec.encode_property(NAME_KEY, self.next_rel(), value) + (-1,))

    def edge(self, a, b, label=0, value=b"", hidden=None):
        """OUT on row a, IN on row b (a, b: the representative rows the entries go to).  hidden: "system" /
        "invisible": an edge the scan skips.  Returns the relation id."""
        rel = self.next_rel()
        if hidden == "system":
            self.rows.setdefault(a, []).append(ec.encode_edge(SYS_EDGE, ec.OUT, b, rel) + (-1,))
            return rel
        inv = hidden == "invisible"
        tid, mult = LABELS[label], MULTS[label]
        self.rows.setdefault(a, []).append(ec.encode_edge(tid, ec.OUT, b, rel, mult, value=value, invisible=inv)
                                           + (-1 if inv else rel,))
        self.rows.setdefault(b, []).append(ec.encode_edge(tid, ec.IN, a, rel, mult, value=value, invisible=inv) + (-1,))
        if not inv:
            self.ends[rel] = (self.canon(a), self.canon(b))
        return rel

    def order(self):
        return sorted(self.rows, key=self.idm.get_key)

    def entries_before(self, v):
        key = self.idm.get_key(v)
        return sum(len(e) for u, e in self.rows.items() if self.idm.get_key(u) < key)

    def pad_to(self, v, end):
        """Short vertex properties on row v until its last entry is entry end - 1 of the store."""
        k = end - self.entries_before(v) - len(self.rows[v])
        assert k >= 0, (v, end, k)
        for _ in range(k):
            self.prop(v)

    def processed(self, row):
        return row in self.live if self.canon(row) == row else True

    def build(self):
        """The store arrays (keys, roff, data, off, vpos, tids, tmult); records the listed edges."""
        data, off, vpos, roff, keys = bytearray(), [0], [], [0], []
        self._listed = []
        for v in self.order():
            keys.append(self.idm.get_key(v))
            for b, vp, rel in sorted(self.rows[v], key=lambda ev: ev[0][: ev[1]]):  # columns in byte order
                if rel >= 0 and self.processed(v):
                    self._listed.append((rel, len(vpos)))
                data += b
                off.append(len(data))
                vpos.append(vp)
            roff.append(len(vpos))
        return (np.array(keys, np.uint64), np.array(roff, np.int64), bytes(data), np.array(off, np.int64),
                np.array(vpos, np.int32), TIDS, TMULT)

    def vertices(self):
        """V in row order."""
        return np.array([u for u in self.order() if u in self.live], np.int64)

    def listed(self):
        """(src, dst, rel, entry index) of the edge list in its order (after build())."""
        rel = np.array([r for r, _ in self._listed], np.int64)
        return (np.array([self.ends[r][0] for r in rel.tolist()], np.int64),
                np.array([self.ends[r][1] for r in rel.tolist()], np.int64), rel,
                np.array([e for _, e in self._listed], np.int64))


def store_random(n=400, m=3000, seed=0, value_of=None, ghosts=0.08, partitioned=4):
    """n vertices (about ghosts * n of them ghost rows, the last `partitioned` vertex-cut with three
    representative rows each) and m edges over all four multiplicities, with self-loops, a bundle of parallel
    MULTI edges, and a few system and invisible edges.  value_of(e, rng) -> the value bytes of edge e."""
    from oracle.oracle import canonical_vertex_id
    rng = np.random.default_rng(seed)
    st = RowStore(5)
    counts = rng.choice(np.arange(1, 1 << 20), n, replace=False)
    vids, reps = [], {}
    for i in range(n):
        c = int(counts[i])
        if i >= n - partitioned:
            canon = canonical_vertex_id((c << 8) | 2, 5)
            others = [x for x in ((((c << 5) + p) << 3) | 2 for p in range(32)) if x != canon]
            reps[i] = [canon] + [others[int(k)] for k in rng.choice(len(others), 2, replace=False)]
            vids.append(canon)
        else:
            vids.append(st.vid(c, int(rng.integers(0, 32)), 4 if rng.integers(0, 8) == 0 else 0))
    ghost = rng.random(n) < ghosts
    ghost[n - partitioned:] = False
    ghost[:8] = False
    for i in range(n):
        st.vertex(vids[i], live=not ghost[i])
        for r in reps.get(i, [])[1:]:
            st.vertex(r, live=False)
        st.prop(vids[i], b"name%d" % i)
        if rng.integers(0, 10) == 0:
            st.edge(vids[i], vids[int(rng.integers(0, n))], hidden="system")
        if rng.integers(0, 10) == 0:
            st.edge(vids[i], vids[int(rng.integers(0, n))], hidden="invisible")

    def row_of(i):
        return reps[i][int(rng.integers(0, 3))] if i in reps else vids[i]

    s, t = rng.integers(0, n, m), rng.integers(0, n, m)
    lab = rng.integers(0, 4, m)
    t[: m // 50] = s[: m // 50]           # self-loops
    s[m // 50: m // 25], t[m // 50: m // 25] = 0, 1  # parallel edges between two live vertices
    lab[: m // 25] = 0                    # MULTI: the multiplicity that allows either
    for e in range(m):
        rel = st.edge(row_of(int(s[e])), row_of(int(t[e])), int(lab[e]), value_of(e, rng) if value_of else b"")
        st.edge_no[rel] = e
    return st


def store_tiles():
    """Rows against the 1024-entry block iterations of edgestore_edges_kernel: a row ending at entry 1024, one
    from there to 2048, then a hub row of VertexExists and 2 * 1024 + 3 OUT entries (block iterations 2, 3 and
    4), then the leaves.  Returns (store, hub)."""
    st = RowStore(5)
    rng = np.random.default_rng(5)
    a, b, hub = st.vertex(st.vid(20)), st.vertex(st.vid(21)), st.vertex(st.vid(30))
    leaves = [st.vertex(st.vid(c)) for c in range(100, 160)]
    ghost = st.vertex(st.vid(170), live=False)
    for k in range(2 * CHUNK + 3):
        st.edge(hub, leaves[int(rng.integers(0, 60))], 0)
    for k in range(300):
        st.edge(leaves[int(rng.integers(0, 60))], leaves[int(rng.integers(0, 60))], int(rng.integers(0, 4)))
    for k in range(5):
        st.edge(a, b)
        st.edge(b, a)
        st.edge(leaves[k], hub)
        st.edge(leaves[k], ghost)
        st.edge(ghost, leaves[k])
    st.edge(hub, hub)
    # the hub's IN entries sort in front of its OUT entries (direction bit): pad the rows in front of it
    st.pad_to(a, CHUNK)
    st.pad_to(b, 2 * CHUNK)
    return st, hub


def store_star(leaves=1500, seed=3):
    """One hub with `leaves` OUT edges to distinct vertices, Double weights from [0.5, 2); every edge has a Long
    and a String of length 0-9 in front of the weight, so the weights start at every residue mod 8."""
    st = RowStore(5)
    rng = np.random.default_rng(seed)
    hub = st.vertex(st.vid(100000))  # the last row: the store ends with the last byte of one of its weights
    w = {}
    for k in range(leaves):
        leaf = st.vertex(st.vid(10 + k))
        x = float(rng.uniform(0.5, 2.0))
        st.edge(hub, leaf, 0, weight_value(ec.DOUBLE, x, rng, pad=k % 10))
        w[leaf] = x
    return st, hub, w


def diamond():
    """s -> a -> t and s -> b -> t, the edge a -> t doubled (two parallel MULTI edges): three shortest paths.
    Returns (store, (s, a, b, t), {name: relation id})."""
    st = RowStore(5)
    s, a, b, t = (st.vertex(st.vid(c)) for c in (10, 11, 12, 13))
    rel = {"sa": st.edge(s, a), "sb": st.edge(s, b), "at1": st.edge(a, t), "at2": st.edge(a, t), "bt": st.edge(b, t)}
    return st, (s, a, b, t), rel


def weight_offsets(store, entries):
    """The byte offset in the store of the first byte of the 8-byte W_KEY value that ends each of `entries`."""
    keys, roff, data, off, vpos, tids, tmult = store
    marker = ec.write_positive(ec.inline_id(W_KEY)) + b"\x00"
    out = []
    for e in np.asarray(entries).tolist():
        end = int(off[e + 1])
        assert data[end - 8 - len(marker):end - 8] == marker, e
        out.append(end - 8)
    return np.array(out, np.int64)


def store_chain(values):
    """v0 -> v1 -> ... with one MULTI edge per element of `values` (the edge's value bytes).  Returns
    (store, vertex ids)."""
    st = RowStore(5)
    vs = [st.vertex(st.vid(10 + i)) for i in range(len(values) + 1)]
    for i, value in enumerate(values):
        st.edge(vs[i], vs[i + 1], 0, value)
    return st, vs
