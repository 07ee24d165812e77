"""The data-dependent paths of the edgestore decoder (janusgraph_amd/csrc/jg_decode.hip), restated on the
CPU, and the stores that reach each of them.

The decoder chooses per block iteration: a 1024-entry iteration of edgestore_edges_kernel stages its bytes
in 16 KB of LDS or reads global memory, and finds an entry's row in a 1024-row LDS window or by a binary
search of global memory; a chunk is staged narrow (u8 lengths and value positions) or wide (i64 offsets)
by its longest entry; decode_edges_kernel stages per 256-entry block.  snapshot_paths / decode_paths /
chunk_width restate those rules, so that every store below can assert that it reaches the path it is
built for (a retuned constant then fails the case instead of quietly emptying it).

This file is the CPU twin of tests/test_gpu_edgestore_paths.py: it builds the same stores, asserts the
same path lists and pins the oracle's snapshot (oracle.edgestore_snapshot) against the graph known by
construction, so that the fixtures and the oracle side are verified without a GPU.
"""
import numpy as np
import pytest

from janusgraph_amd.idmanager import IDManager
from oracle import edgecodec as ec
from test_slice_cap import VERTEX_EXISTS, store_from_rows

# jg_decode.hip, in one place:
CHUNK = 1024         # kChunk = kEpt * kBlock: entries per block iteration of edgestore_edges_kernel
STAGE_WORDS = 4096   # kStageWords: dwords of the LDS stage (stage_entries)
ROW_WIN = 1024       # kRowWin: rows of the LDS row window (edgestore_edges_kernel)
WIDE_LEN = 256       # EdgestoreDecoder::add: a chunk holding an entry this long is staged wide
DECODE_BLOCK = 256   # kBlock: entries per block iteration of decode_edges_kernel

LABELS = [ec.schema_id(c, "user_edge") for c in (11, 12, 13, 14, 15)]
MULTS = [ec.MULTI, ec.SIMPLE, ec.ONE2MANY, ec.MANY2ONE, ec.ONE2ONE]
TIDS = np.array(LABELS[1:], np.int64)
TMULT = np.array(MULTS[1:], np.int8)
NAME_KEY = ec.schema_id(5, "user_key")
FILL_KEY = ec.schema_id(6, "user_key")
BAD_ENTRY = ec.write_relation_type(LABELS[0], True, ec.OUT) + b"\x01\x02"  # its backward id reaches position 0


def _stage(off, e0, e_end):
    return "staged" if ((int(off[e_end]) - (int(off[e0]) & ~3) + 3) >> 2) <= STAGE_WORDS else "global"


def snapshot_paths(row_off, entry_off):
    """Per 1024-entry block iteration of edgestore_edges_kernel over one chunk (the arrays as the decoder
    sees them: row offsets from 0): (stage path, row path, rows in [r0, r1))."""
    roff, off = np.asarray(row_off, np.int64), np.asarray(entry_off, np.int64)
    nrows, nent = len(roff) - 1, len(off) - 1

    def row_of(e):  # block_rows_kernel: the row holding entry e (never an empty one)
        return int(np.searchsorted(roff, e, side="right")) - 1

    out = []
    for e0 in range(0, nent, CHUNK):
        e_end = min(e0 + CHUNK, nent)
        r0 = row_of(e0)
        r1 = row_of(e_end) + 1 if e_end < nent else nrows
        out.append((_stage(off, e0, e_end), "window" if r1 - r0 <= ROW_WIN else "search", r1 - r0))
    return out


def decode_paths(entry_off):
    """Per 256-entry block of decode_edges_kernel: the stage path."""
    off = np.asarray(entry_off, np.int64)
    n = len(off) - 1
    return [_stage(off, e0, min(e0 + DECODE_BLOCK, n)) for e0 in range(0, n, DECODE_BLOCK)]


def chunk_width(entry_off):
    off = np.asarray(entry_off, np.int64)
    return "wide" if len(off) > 1 and int(np.max(np.diff(off))) >= WIDE_LEN else "narrow"


def stage_starts(entry_off):
    """off[e0] % 4 of every block iteration (the aligned-down start adds it to the word count)."""
    off = np.asarray(entry_off, np.int64)
    return [int(off[e0]) % 4 for e0 in range(0, len(off) - 1, CHUNK)]


def _insert_row(store, key, ents):
    """The store with one more row (key, [(entry bytes, value position, ...)]) at its place in key order."""
    keys, roff, data, off, vpos, tids, tmult = store
    r = int(np.searchsorted(keys, np.uint64(key)))
    e = int(roff[r])
    b = int(off[e])
    blob = b"".join(x[0] for x in ents)
    ends = b + np.cumsum([len(x[0]) for x in ents], dtype=np.int64)
    return (np.insert(keys, r, np.uint64(key)), np.concatenate([roff[:r + 1], roff[r:] + len(ents)]),
            data[:b] + blob + data[b:], np.concatenate([off[:e + 1], ends, off[e + 1:] + len(blob)]),
            np.concatenate([vpos[:e], np.array([x[1] for x in ents], np.int32), vpos[e:]]), tids, tmult)


class Store:
    """Edgestore rows written as JanusGraph lays them out, with the graph they hold known by construction.
    Rows are keyed by vertex id (vid(count, partition, suffix)); the key order is (partition, count,
    suffix), the entries of a row sort by column.  Schema rows (odd keys) are (key, entries) pairs."""

    def __init__(self, partition_bits=5):
        self.pbits = partition_bits
        self.idm = IDManager(partition_bits)
        self.rows = {}      # row vertex id -> [(entry bytes, value position, tag)]
        self.live = set()   # canonical ids whose row starts with VertexExists
        self.edges = []     # (row of the OUT entry, canonical source, canonical target)
        self.schema = []    # (odd key, [(entry bytes, value position)])
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

    def row(self, v):
        return self.rows.setdefault(v, [])

    def vertex(self, v, live=True):
        """A row; live: VertexExists on it (a row without it is a ghost, or a non-canonical representative)."""
        self.row(v)
        if live:
            self.rows[v].append(ec.encode_property(VERTEX_EXISTS, self.next_rel(), b"\x01") + (None,))
            self.live.add(v)
        return v

    def prop(self, v, value=b"x", key=NAME_KEY, tag=None):
        self.row(v).append(ec.encode_property(key, self.next_rel(), value) + (tag,))

    def out_entry(self, a, b, label=LABELS[0], mult=ec.MULTI, value=b"", sort_key=b""):
        rel = self.next_rel()
        self.row(a).append(ec.encode_edge(label, ec.OUT, b, rel, mult, sort_key=sort_key, value=value) + (None,))
        self.edges.append((a, self.canon(a), self.canon(b)))
        return rel

    def edge(self, a, b, label=LABELS[0], mult=ec.MULTI, value=b""):
        """OUT on a's row, IN on b's row (a and b: the representative rows the entries go to)."""
        rel = self.out_entry(a, b, label, mult, value)
        self.row(b).append(ec.encode_edge(label, ec.IN, a, rel, mult, value=value) + (None,))

    def _sorted(self, v):
        return sorted(self.rows[v], key=lambda ev: ev[0][: ev[1]])

    def order(self):
        return sorted(self.rows, key=self.idm.get_key)

    def _all_rows(self):
        """[(key, entries in column order)] of every row, vertex and schema, in key order."""
        rows = [(self.idm.get_key(v), self._sorted(v)) for v in self.rows]
        rows += [(k, [tuple(e) + (None,) * (3 - len(e)) for e in ents]) for k, ents in self.schema]
        return sorted(rows, key=lambda r: r[0])

    def entries_before(self, v):
        """Entries of the store in front of row v."""
        key = self.idm.get_key(v)
        return sum(len(ents) for k, ents in self._all_rows() if k < key)

    def pad_to(self, v, end):
        """Short properties on row v until its last entry is entry end - 1 of the store."""
        k = end - self.entries_before(v) - len(self.rows[v])
        assert k >= 0, (v, end, k)
        for _ in range(k):
            self.prop(v)

    def build(self):
        rows = {v: [(b, vp) for b, vp, _ in ents] for v, ents in self.rows.items()}
        store = store_from_rows(rows, self.pbits, TIDS, TMULT)
        for key, ents in sorted(self.schema):  # odd keys: wherever they sort among the vertex rows
            store = _insert_row(store, key, ents)
        return store

    def tagged(self):
        """{tag: entry index in the built store}"""
        out, e = {}, 0
        for _, ents in self._all_rows():
            for _, _, tag in ents:
                if tag is not None:
                    out[tag] = e
                e += 1
        return out

    def processed(self, row):
        """The scan decodes a row's entries if it is a live vertex's own row or a non-canonical
        representative (never a ghost)."""
        return row in self.live if self.canon(row) == row else True

    def truth(self):
        """(V in row order, src, dst) of the snapshot, and its ghost edges: OUT entries on processed rows
        with an endpoint outside V."""
        v = [u for u in self.order() if u in self.live]
        kept = [(s, t) for row, s, t in self.edges if self.processed(row)]
        inside = [(s, t) for s, t in kept if s in self.live and t in self.live]
        return (np.array(v, np.int64), np.array([s for s, _ in inside], np.int64),
                np.array([t for _, t in inside], np.int64)), len(kept) - len(inside)


def add_mixed(st, rng, counts, partitions=(0,), nedges=400, cut_count=None, cut_parts=None, value_len=0,
              cut_edges_on=None):
    """The things every case carries: live vertices over `partitions` with random MULTI edges (self-loops
    and multi-edges among them), two ghost rows with edges in and out, an edge of each of the four
    non-MULTI multiplicities, and (cut_count) one vertex-cut vertex whose representative rows in
    cut_parts share its edges (those in cut_edges_on alone, if given; the canonical row always holds
    VertexExists).  One edge in twenty carries a value of up to value_len bytes.  Returns the live vertex ids."""
    vs = [st.vertex(st.vid(c, partitions[i % len(partitions)])) for i, c in enumerate(counts)]
    n = len(vs)
    ghosts = [st.vertex(st.vid(counts[-1] + 1 + i, partitions[0]), live=False) for i in range(2)]

    def val():
        if not value_len or rng.integers(0, 20):
            return b""
        return rng.integers(0, 256, int(rng.integers(1, value_len + 1)), dtype=np.uint8).tobytes()

    for _ in range(nedges):
        st.edge(vs[int(rng.integers(0, n))], vs[int(rng.integers(0, n))], value=val())
    for i in range(6):
        st.edge(vs[i], vs[i])          # self-loops
        st.edge(vs[i], vs[n - 1 - i])  # multi-edges
        st.edge(vs[i], vs[n - 1 - i])
    for i, gh in enumerate(ghosts):
        st.edge(gh, vs[i])
        st.edge(vs[i + 2], gh)
    st.edge(vs[0], vs[1], LABELS[1], MULTS[1])  # SIMPLE
    st.edge(vs[0], vs[2], LABELS[1], MULTS[1])
    st.edge(vs[0], vs[3], LABELS[2], MULTS[2])  # ONE2MANY: one in-edge per vertex
    st.edge(vs[0], vs[4], LABELS[2], MULTS[2])
    st.edge(vs[1], vs[0], LABELS[3], MULTS[3])  # MANY2ONE: one out-edge per vertex
    st.edge(vs[2], vs[0], LABELS[3], MULTS[3])
    st.edge(vs[3], vs[4], LABELS[4], MULTS[4])  # ONE2ONE
    st.edge(vs[4], vs[5], LABELS[4], MULTS[4])
    if cut_count is not None:
        reps = [st.vid(cut_count, p, 2) for p in cut_parts]
        canon = st.canon(reps[0])
        assert canon in reps and all(st.canon(r) == canon for r in reps)
        for r in reps:
            st.vertex(r, live=r == canon)
        er = [st.vid(cut_count, p, 2) for p in (cut_edges_on or cut_parts)]
        for i in range(12):
            st.edge(er[i % len(er)], vs[i])
            st.edge(vs[i + 1], er[(i + 1) % len(er)])
        st.edge(er[0], er[-1])  # a self-loop of the cut vertex (across two representatives)
    return vs


def cut_count_for(pbits, partition):
    """A count whose canonical partition (the xor of its pbits-wide groups) is `partition`."""
    c = (1 << pbits) | ((1 ^ partition) & ((1 << pbits) - 1)) if pbits else 1
    from oracle.oracle import canonical_vertex_id
    v = canonical_vertex_id((c << (pbits + 3)) | 2, pbits)
    assert (v >> 3) & ((1 << pbits) - 1) == partition
    return c


# ---------------------------------------------------------------- A: the row window

def store_row_window(bad_on=None):
    """Rows in key order (5 partition bits):
      partition 0 and 1: 3100 one-entry rows but for one two-entry row: live isolated vertices, four
        ghosts whose single entry is an OUT edge, the vertex-cut vertex's canonical row (VertexExists
        alone, partition 0) and a representative holding one OUT edge (partition 1); a schema row in front.
        Block iterations 0 and 1 span 1025 rows (search), iteration 2 exactly 1024 (window).
      partition 2, 3: ordinary rows; partition 30: the third representative, with edges in and out.
      partition 31: 1024 one-entry rows padded to fill the last block iteration, then 4 empty rows of live
        keys: the last iteration spans 1028 rows with r1 = nrows.
    bad_on: None, or the rows that get BAD_ENTRY: 'ghost+schema' (ignored rows: a schema row's only entry
    and a ghost row's second), 'rep' (a kept row's only entry)."""
    st = Store(5)
    rng = np.random.default_rng(21)
    cc = cut_count_for(5, 0)
    canon, rep1, rep30 = st.vid(cc, 0, 2), st.vid(cc, 1, 2), st.vid(cc, 30, 2)
    assert st.canon(rep1) == canon
    mixed = add_mixed(st, rng, range(5000, 5120), partitions=(2, 3), nedges=500, cut_count=cc, cut_parts=(0, 1, 30),
                      cut_edges_on=(30,))
    assert len(st.rows[canon]) == 1 and st.rows[rep1] == [] and len(st.rows[rep30]) > 20
    if bad_on == "rep":
        st.rows[rep1].append((BAD_ENTRY, len(BAD_ENTRY), "bad"))
    else:
        st.out_entry(rep1, mixed[7])
    st.schema.append((ec.schema_id(1, "user_edge"), [ec.encode_property(NAME_KEY, 5, b"schema")]))
    iso = []
    for p in (0, 1):
        for c in range(100, 100 + 1548):
            iso.append(st.vid(c, p))
    ghost_at = {60, 900, 1500, 2040}
    two_at = 2100
    for i, v in enumerate(iso):
        if i in ghost_at:
            st.vertex(v, live=False)
            if bad_on == "ghost+schema" and i == 900:
                # behind a property: the ghost rule itself decodes a row's first entry (as isGhostVertex parses
                # it) and refuses a malformed one.  The empty row keeps the iteration at 1025 rows.
                st.prop(v)
                st.row(v).append((BAD_ENTRY, len(BAD_ENTRY), "bad"))
                st.vertex(v | 4, live=False)
            else:
                st.out_entry(v, mixed[i % 50])
        else:
            st.vertex(v)
            if i == two_at:
                st.out_entry(v, mixed[3])
    if bad_on == "ghost+schema":
        st.schema.append((ec.schema_id(2, "user_edge"), [(BAD_ENTRY, len(BAD_ENTRY))]))
    for c in range(100, 100 + 1024):
        st.vertex(st.vid(c, 31))
    total = sum(len(r) for r in st.rows.values()) + sum(len(e) for _, e in st.schema)
    last_ordinary = max((v for v in st.rows if (v >> 3) & 31 == 30), key=st.idm.get_key)
    st.pad_to(last_ordinary, -(-(total - 1024) // CHUNK) * CHUNK)
    for c in range(2000, 2004):
        st.vertex(st.vid(c, 31), live=False)  # empty rows of live keys: dropped as ghosts
    return st


ROW_WINDOW_PATHS = ["search", "search", "window"]


def check_row_window_paths(store):
    keys, roff, data, off, vpos, _, _ = store
    paths = snapshot_paths(roff, off)
    assert [p[1] for p in paths[:3]] == ROW_WINDOW_PATHS
    assert paths[0][2] == ROW_WIN + 1 and paths[1][2] == ROW_WIN + 1 and paths[2][2] == ROW_WIN
    assert all(p[1] == "window" for p in paths[2:-1])
    assert paths[-1][1] == "search" and paths[-1][2] == ROW_WIN + 4 and len(vpos) % CHUNK == 0
    assert all(p[0] == "staged" for p in paths) and len(vpos) <= 12000
    return paths


# ---------------------------------------------------------------- B: rows against block iterations

HUB_START = 2 * CHUNK + 900


def store_alignment(limit=None):
    """Key order: an empty row first; a row ending at entry 1024, one starting there and ending at 2048, an
    empty row on that boundary; a hub row from entry 2948 over four block iterations (multi-edges in and
    out); two rows whose EDGE slices hold exactly `limit` and `limit + 1` entries; the leaves and the
    mixed rows; an empty row last.  The empty rows are live keys: the scan drops them as ghosts."""
    st = Store(5)
    rng = np.random.default_rng(22)
    first = st.vertex(st.vid(10), live=False)
    a, b, on_edge = st.vertex(st.vid(20)), st.vertex(st.vid(21)), st.vertex(st.vid(22), live=False)
    pre = st.vertex(st.vid(23))
    hub = st.vertex(st.vid(30))
    leaves = add_mixed(st, rng, range(100, 180), nedges=300, cut_count=cut_count_for(5, 3), cut_parts=(3, 9, 17))
    for k in range(1100):
        st.edge(hub, leaves[int(rng.integers(0, 40))])
        st.edge(leaves[int(rng.integers(0, 40))], hub)
    for k in range(5):
        st.edge(a, b)
        st.edge(b, pre)
    if limit:
        exact, over = st.vertex(st.vid(40)), st.vertex(st.vid(41))
        for k in range(limit):
            st.edge(exact, leaves[40 + k % 30])
        for k in range(limit + 1):
            st.edge(leaves[40 + k % 30], over) if k % 2 else st.edge(over, leaves[40 + k % 30])
    last = st.vertex(st.vid(9000, 31), live=False)
    st.pad_to(a, CHUNK)
    st.pad_to(b, 2 * CHUNK)
    st.pad_to(pre, HUB_START)
    assert st.entries_before(first) == 0 and st.entries_before(on_edge) == 2 * CHUNK and st.rows[last] == []
    return st, hub


def check_alignment_paths(st, hub, store):
    keys, roff, data, off, vpos, _, _ = store
    h = st.order().index(hub)
    assert roff[h] == HUB_START and roff[h + 1] > 5 * CHUNK  # block iterations 2, 3, 4 and 5
    assert CHUNK in roff and 2 * CHUNK in roff
    assert roff[0] == roff[1] and roff[-1] == roff[-2]  # empty rows first and last
    r = int(np.searchsorted(roff, 2 * CHUNK))
    assert roff[r] == roff[r + 1] == roff[r - 1] + CHUNK  # a row of exactly one iteration, then the empty row
    paths = snapshot_paths(roff, off)
    assert all(p[1] == "window" for p in paths) and paths[3][2] == 1 and len(vpos) <= 12000
    return paths


def store_tiny(nentries, nrows_empty=0):
    """Exactly nentries entries (two live vertices, edges between them, short properties); nentries 0:
    nrows_empty empty rows."""
    st = Store(5)
    if nentries == 0:
        for c in range(nrows_empty):
            st.vertex(st.vid(10 + c), live=False)
        return st
    a = st.vertex(st.vid(10))
    if nentries >= 6:
        b = st.vertex(st.vid(11))
        st.edge(a, b)
        st.edge(b, b)
        st.pad_to(b, nentries)
    return st


# ---------------------------------------------------------------- C: the stage limit

# (words of the block iteration, off % 4 at which the next one starts); None: as the entries fall
STAGE_PLAN = [(None, 1), (STAGE_WORDS, 2), (STAGE_WORDS + 1, 3), (STAGE_WORDS, 0), (3000, 0), (6000, 1), (None, None)]


STAGE_SCHEMA_KEY = (621 << 3) | 1  # an odd key behind the rows of count 620 (partition 0): iteration 5


def store_stage_limit(bad_on=None, hub=False):
    """Every vertex carries a filler property (a long user_key string); the edges carry values of up to
    60 bytes.  The fillers of each 1024-entry block iteration are sized so that iteration 1 takes exactly
    4096 words (from a start at off % 4 = 1), iteration 2 4097 (start 2), iteration 3 4096 (start 3),
    iteration 4 stays small and iteration 5 is far above the stage: staged and global side by side.
    bad_on: 'live': BAD_ENTRY on a live row of iteration 5; 'ghost+schema': on a ghost row there (behind
    its filler) and as the only entry of a schema row (STAGE_SCHEMA_KEY) behind it.
    hub: a last partition-0 row of 1101 entries and more than 16 KB (for the one-shot chunker's limits)."""
    st = Store(5)
    rng = np.random.default_rng(23)
    cc = cut_count_for(5, 0)
    vs = add_mixed(st, rng, range(100, 700), nedges=2700, cut_count=cc, cut_parts=(0, 1, 2), value_len=40)
    ghost = st.vertex(st.vid(620, 0, 4), live=False)  # a ghost row inside iteration 5
    st.edge(ghost, vs[0])
    st.edge(vs[1], ghost)
    if hub:
        h = st.vertex(st.vid(800))
        for k in range(1100):
            st.edge(h, vs[k % 600], value=bytes(rng.integers(0, 256, 10, dtype=np.uint8)))
    for v in list(st.rows):
        st.prop(v, b"", FILL_KEY, tag=("fill", v))
    if bad_on:
        st.row(ghost if bad_on == "ghost+schema" else vs[520]).append((BAD_ENTRY, len(BAD_ENTRY), "bad"))
    if bad_on == "ghost+schema":
        st.schema.append((STAGE_SCHEMA_KEY, [(BAD_ENTRY, len(BAD_ENTRY), "bad in schema")]))
    fills = st.tagged()
    assert fills.pop("bad", 5 * CHUNK) // CHUNK == 5 and fills.pop("bad in schema", 5 * CHUNK) // CHUNK == 5
    nent = sum(len(ents) for _, ents in st._all_rows())
    size = {tag: 0 for tag in fills}
    for k, (words, nxt) in enumerate(STAGE_PLAN):
        e0, e_end = k * CHUNK, min((k + 1) * CHUNK, nent)
        mine = [t for t, e in fills.items() if e0 <= e < e_end]
        _, _, _, off, _, _, _ = st.build()
        start = int(off[e0]) % 4
        span = int(off[e_end] - off[e0])
        if words is None and nxt is None:
            break
        if words is None:
            words = (span + start + 3 + 3) >> 2
        want = next(s for s in range(4 * words - 3, 4 * words + 1) if s % 4 == nxt) - start - span
        assert 0 <= want <= 240 * len(mine), (k, want, len(mine))
        for t in mine:
            size[t] = min(240, want)
            want -= size[t]
            row = st.rows[t[1]]
            i = next(i for i, e in enumerate(row) if e[2] == t)
            col = row[i][0][: row[i][1]]
            row[i] = (col + bytes(rng.integers(0, 256, size[t], dtype=np.uint8)), row[i][1], t)
    return st


def check_stage_paths(store):
    keys, roff, data, off, vpos, _, _ = store
    paths = snapshot_paths(roff, off)
    words = [((int(off[min(e0 + CHUNK, len(vpos))]) - (int(off[e0]) & ~3) + 3) >> 2) for e0 in range(0, len(vpos), CHUNK)]
    assert words[1] == STAGE_WORDS and words[2] == STAGE_WORDS + 1 and words[3] == STAGE_WORDS
    assert [p[0] for p in paths[:6]] == ["staged", "staged", "global", "staged", "staged", "global"]
    assert stage_starts(off)[:6] == [0, 1, 2, 3, 0, 0] and len(vpos) <= 12000
    assert chunk_width(off) == "narrow"
    return paths


def one_shot_chunks(row_off, entry_off, max_entries, max_bytes):
    """add_in_chunks restated: the row bounds of the chunks jg_graph_build_edgestore cuts (whole rows, at
    most max_entries entries and max_bytes bytes each; a larger row is a chunk of its own)."""
    roff, off = np.asarray(row_off, np.int64), np.asarray(entry_off, np.int64)
    nrows, bounds, lo = len(roff) - 1, [0], 0
    while lo < nrows:
        hi = lo + 1
        while hi < nrows and roff[hi + 1] - roff[lo] <= max_entries and off[roff[hi + 1]] - off[roff[lo]] <= max_bytes:
            hi += 1
        bounds.append(hi)
        lo = hi
    return bounds


CHUNKER_LIMITS = [(1000, 1 << 30), (4 << 20, 16 << 10)]
CHUNKER_DEFAULTS = (4 << 20, 64 << 20)  # add_in_chunks: edgestore_chunk_entries, edgestore_chunk_bytes


def check_chunker(store, max_entries, max_bytes):
    """The limits cut the store into many chunks, the hub row alone in one above both limits' reach."""
    keys, roff, data, off, vpos, _, _ = store
    bounds = one_shot_chunks(roff, off, max_entries, max_bytes)
    ent = np.diff(roff[bounds])
    nbytes = np.diff(off[roff[bounds]])
    big = (ent > max_entries) | (nbytes > max_bytes)
    assert len(bounds) > 8 and big.sum() == 1 and np.diff(bounds)[big][0] == 1
    assert np.all(ent[~big] <= max_entries) and np.all(nbytes[~big] <= max_bytes)
    if max_bytes < (1 << 30):  # the byte limit cuts first: no chunk comes near the entry limit
        assert ent.max() < max_entries and ent[big][0] > 1000 and nbytes[big][0] > max_bytes
    return bounds


# ---------------------------------------------------------------- D: narrow and wide

def store_width(nentries, longest):
    """nentries entries whose longest is `longest` bytes (255: narrow, with one entry whose value position
    is 255; 256: wide)."""
    st = Store(5)
    rng = np.random.default_rng(nentries + longest)
    vs = add_mixed(st, rng, range(100, 160), nedges=600, cut_count=cut_count_for(5, 2), cut_parts=(2, 5, 11))
    if longest == WIDE_LEN - 1:  # a MULTI edge with a sort key: column = entry, its ids end at 255
        e, vp = ec.encode_edge(LABELS[0], ec.OUT, vs[9], st.next_rel(), sort_key=bytes(248))
        skey = bytes(248 - (len(e) - 255))
        st.out_entry(vs[8], vs[9], sort_key=skey)
        assert st.rows[vs[8]][-1][1] == 255 == len(st.rows[vs[8]][-1][0])
    col = len(ec.encode_property(NAME_KEY, st.rel + 1, b"")[0])
    st.prop(vs[20], bytes(rng.integers(0, 256, longest - col, dtype=np.uint8)))
    st.pad_to(max(st.rows, key=st.idm.get_key), nentries)
    return st


def check_width(store, nentries, longest):
    off, vpos = store[3], store[4]
    assert len(vpos) == nentries and int(np.max(np.diff(off))) == longest
    assert chunk_width(off) == ("narrow" if longest < WIDE_LEN else "wide")
    if longest == WIDE_LEN - 1:
        assert int(np.max(vpos)) == 255


def with_entry_base(chunk, base=5):
    """The chunk with `base` unused leading bytes: entry_off[0] = base."""
    keys, roff, data, off, vpos = chunk[:5]
    return keys, roff, b"\xaa" * base + bytes(data), np.asarray(off) + base, vpos


# ---------------------------------------------------------------- E: slot reuse

def store_slot_reuse():
    """Five runs of rows for the builder's chunks: large narrow, small wide, an empty chunk (two empty
    rows), tiny narrow, large wide.  Returns the store and the row bounds of the chunks."""
    st = Store(5)
    rng = np.random.default_rng(25)
    a = add_mixed(st, rng, range(100, 260), nedges=1300, cut_count=cut_count_for(5, 1), cut_parts=(1, 8, 20))
    b = [st.vertex(st.vid(c)) for c in range(1000, 1010)]
    empty = [st.vertex(st.vid(c), live=False) for c in (2000, 2001)]
    c = [st.vertex(st.vid(c)) for c in range(3000, 3003)]
    d = [st.vertex(st.vid(c)) for c in range(4000, 4160)]
    for k in range(30):
        st.edge(b[k % 10], a[k])
        st.edge(c[k % 3], d[k])
        st.edge(a[k], c[k % 3])
    for k in range(1300):
        st.edge(d[int(rng.integers(0, 160))], d[int(rng.integers(0, 160))])
        st.edge(d[int(rng.integers(0, 160))], a[int(rng.integers(0, 160))])
    st.prop(b[4], bytes(rng.integers(0, 256, 300, dtype=np.uint8)))
    st.prop(d[100], bytes(rng.integers(0, 256, 600, dtype=np.uint8)))
    order = st.order()
    bounds = [0] + [order.index(v) for v in (b[0], empty[0], c[0], d[0])] + [len(order)]
    # the cut vertex's representatives in partitions 1, 8 and 20 sort behind every partition-0 row
    assert bounds == sorted(bounds)
    return st, bounds


SLOT_WIDTHS = ["narrow", "wide", "narrow", "narrow", "wide"]


def check_slot_reuse(store, bounds):
    from test_gpu_builder import row_chunks
    chunks = row_chunks(store, bounds)
    assert [chunk_width(ch[3]) for ch in chunks] == SLOT_WIDTHS
    n = [len(ch[4]) for ch in chunks]
    assert n[2] == 0 and len(chunks[2][0]) == 2 and n[3] < 100 and n[1] < 200 and n[0] > 2 * CHUNK and n[4] > 2 * CHUNK
    assert len(store[4]) <= 12000
    return chunks


# ---------------------------------------------------------------- G: partition bits

def store_partition_bits(pbits, cut=True):
    st = Store(pbits)
    rng = np.random.default_rng(26 + pbits)
    nparts = 1 << pbits
    parts = sorted({0, nparts - 1, nparts // 2, min(3, nparts - 1)})
    cut_parts = (0, nparts - 1) if pbits == 1 else (0, nparts // 2, nparts - 1)
    cc = None
    if cut:
        cc = cut_count_for(pbits, cut_parts[0])
    add_mixed(st, rng, range(100, 400), partitions=parts, nedges=1500, cut_count=cc, cut_parts=cut_parts)
    return st


# ---------------------------------------------------------------- the checks of this file

def assert_oracle_matches_construction(oracle_lib, st, store):
    keys, roff, data, off, vpos, tids, tmult = store
    (v, s, t), ghost_edges = st.truth()
    gv, gs, gt = oracle_lib.edgestore_snapshot(keys, roff, data, off, vpos, tids, tmult, partition_bits=st.pbits)
    assert np.array_equal(gv, v)
    inside = np.isin(gs, gv) & np.isin(gt, gv)
    assert int((~inside).sum()) == ghost_edges
    assert sorted(zip(gs[inside].tolist(), gt[inside].tolist())) == sorted(zip(s.tolist(), t.tolist()))
    return gv, gs, gt


def test_row_window_store(oracle_lib):
    st = store_row_window()
    store = st.build()
    paths = check_row_window_paths(store)
    assert {p[1] for p in paths} == {"search", "window"}
    gv, gs, gt = assert_oracle_matches_construction(oracle_lib, st, store)
    # the search-path iterations decide edges: the ghosts' OUT entries are dropped, the representative's kept
    canon = st.canon(st.vid(cut_count_for(5, 0), 1, 2))
    assert canon in gv and int((gs == canon).sum()) >= 2
    st2 = store_row_window("ghost+schema")
    check_row_window_paths(st2.build())
    assert_oracle_matches_construction(oracle_lib, st2, st2.build())
    check_row_window_paths(store_row_window("rep").build())


def test_alignment_store(oracle_lib):
    for limit in (None, 300):
        st, hub = store_alignment(limit)
        store = st.build()
        check_alignment_paths(st, hub, store)
        assert_oracle_matches_construction(oracle_lib, st, store)


@pytest.mark.parametrize("nentries", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_tiny_stores(oracle_lib, nentries):
    st = store_tiny(nentries, 3)
    store = st.build()
    assert len(store[4]) == nentries and len(store[0]) > 0
    assert len(snapshot_paths(store[1], store[3])) == -(-nentries // CHUNK)
    assert_oracle_matches_construction(oracle_lib, st, store)


def test_stage_limit_store(oracle_lib):
    st = store_stage_limit()
    store = st.build()
    paths = check_stage_paths(store)
    assert {p[0] for p in paths} == {"staged", "global"}
    assert_oracle_matches_construction(oracle_lib, st, store)
    check_stage_paths(store_stage_limit("live").build())
    st = store_stage_limit("ghost+schema")
    store = st.build()
    paths = check_stage_paths(store)
    r = int(np.flatnonzero(store[0] == np.uint64(STAGE_SCHEMA_KEY))[0])
    assert store[1][r + 1] - store[1][r] == 1 and paths[store[1][r] // CHUNK][0] == "global"
    assert_oracle_matches_construction(oracle_lib, st, store)


@pytest.mark.parametrize("longest", [WIDE_LEN - 1, WIDE_LEN])
@pytest.mark.parametrize("nentries", [2047, 2048, 2049])
def test_width_stores(oracle_lib, nentries, longest):
    st = store_width(nentries, longest)
    store = st.build()
    check_width(store, nentries, longest)
    assert_oracle_matches_construction(oracle_lib, st, store)
    based = with_entry_base(store)
    assert based[3][0] == 5 and chunk_width(based[3]) == chunk_width(store[3])  # the nonzero entry base


def test_slot_reuse_store(oracle_lib):
    st, bounds = store_slot_reuse()
    store = st.build()
    check_slot_reuse(store, bounds)
    assert_oracle_matches_construction(oracle_lib, st, store)


@pytest.mark.parametrize("pbits,cut", [(1, True), (16, True), (0, False)])
def test_partition_bits_stores(oracle_lib, pbits, cut):
    st = store_partition_bits(pbits, cut)
    assert_oracle_matches_construction(oracle_lib, st, st.build())


def test_no_partition_bits_refuse_a_cut_vertex(oracle_lib):
    st = store_partition_bits(0, False)
    st.vertex(st.vid(77, 0, 2))
    keys, roff, data, off, vpos, tids, tmult = st.build()
    with pytest.raises(ValueError):
        oracle_lib.edgestore_snapshot(keys, roff, data, off, vpos, tids, tmult, partition_bits=0)


def test_chunker_store(oracle_lib):
    st = store_stage_limit(hub=True)
    store = st.build()
    check_stage_paths(store)
    for max_entries, max_bytes in CHUNKER_LIMITS:
        check_chunker(store, max_entries, max_bytes)
    assert one_shot_chunks(store[1], store[3], *CHUNKER_DEFAULTS) == [0, len(store[0])]
    assert_oracle_matches_construction(oracle_lib, st, store)


def test_path_predicates_at_their_limits():
    # stage: 4096 words staged, 4097 not; the start's misalignment counts
    assert _stage([0, 4 * STAGE_WORDS], 0, 1) == "staged" and _stage([0, 4 * STAGE_WORDS + 1], 0, 1) == "global"
    assert _stage([3, 4 * STAGE_WORDS], 0, 1) == "staged" and _stage([3, 4 * STAGE_WORDS + 1], 0, 1) == "global"
    assert _stage([4, 4 * STAGE_WORDS + 4], 0, 1) == "staged"
    # rows: 1024 one-entry rows and the row of the next iteration's first entry = 1025
    assert snapshot_paths(np.arange(2 * CHUNK + 1), np.arange(2 * CHUNK + 1))[0][1:] == ("search", ROW_WIN + 1)
    assert snapshot_paths(np.arange(2 * CHUNK + 1), np.arange(2 * CHUNK + 1))[1][1:] == ("window", ROW_WIN)
    roff = np.concatenate([np.arange(CHUNK + 1), [CHUNK]])  # e_end == nent: r1 = nrows, an empty row counted
    assert snapshot_paths(roff, np.arange(CHUNK + 1))[0][1:] == ("search", ROW_WIN + 1)
    assert chunk_width([0, 255]) == "narrow" and chunk_width([0, 256]) == "wide"
    assert decode_paths(np.arange(0, 65 * 600, 65))[:2] == ["global", "global"]
    assert decode_paths(np.arange(0, 64 * 600, 64))[0] == "staged"


# ---------------------------------------------------------------- jg_decode_edges batches

def _edge(label, direction, other, rel, mult=ec.MULTI, value=b"", invisible=False, sort_key=b""):
    b, vp = ec.encode_edge(label, direction, other, rel, mult, sort_key=sort_key, value=value, invisible=invisible)
    return b, vp, (label, direction, other, rel)


def _prop(key, rel, value):
    b, vp = ec.encode_property(key, rel, value)
    return b, vp, (key, 2, -1, -1)


def _random_entry(rng, heavy):
    """One entry of a random kind; heavy: property values of 60 to 250 bytes, edge values up to 200."""
    kind = int(rng.integers(0, 8))
    vlen = int(rng.integers(60, 251)) if heavy else int(rng.integers(0, 6))
    elen = int(rng.integers(0, 201)) if heavy else 0
    val = bytes(rng.integers(0, 256, vlen, dtype=np.uint8))
    eval_ = bytes(rng.integers(0, 256, elen, dtype=np.uint8))
    other, rel = int(rng.integers(1, 1 << 40)) << 8, int(rng.integers(1, 1 << 30))
    direction = int(rng.integers(0, 2))
    if kind == 0:
        return _prop(ec.schema_id(int(rng.integers(1, 500)), "user_key"), rel, val)
    if kind == 1:
        return _prop(ec.schema_id(int(rng.integers(1, 40)), "system_key"), rel, val)
    if kind == 2:
        sys_edge = ec.schema_id(int(rng.integers(1, 40)), "system_edge")
        b, vp = ec.encode_edge(sys_edge, direction, other, rel, value=eval_)
        return b, vp, (sys_edge, 3, -1, -1)
    if kind == 3:
        return _edge(LABELS[0], direction, other, rel, value=eval_, invisible=True)
    m = int(rng.integers(0, 5))
    return _edge(LABELS[m], direction, other, rel, MULTS[m], value=eval_)


def _pack(entries):
    data, off, vpos = bytearray(), [0], []
    for b, vp, _ in entries:
        data += b
        off.append(len(data))
        vpos.append(vp)
    want = np.array([x for _, _, x in entries], np.int64).reshape(-1, 4)
    return bytes(data), np.array(off, np.int64), np.array(vpos, np.int32), want


DECODE_MIXED_PATHS = ["staged", "global", "staged", "global", "global", "staged", "global", "staged", "staged", "staged"]


def decode_mixed_batch():
    """2381 entries of every kind; the 256-entry blocks named global hold long values.  The last entry of
    each block is a property sized so that the next block starts at off % 4 = its index % 4."""
    rng = np.random.default_rng(31)
    entries, nbytes = [], 0
    n = DECODE_BLOCK * (len(DECODE_MIXED_PATHS) - 1) + 77
    for i in range(n):
        blk = i // DECODE_BLOCK
        if i % DECODE_BLOCK == DECODE_BLOCK - 1:
            col = len(ec.encode_property(NAME_KEY, 7, b"")[0])
            e = _prop(NAME_KEY, 7, bytes(((blk + 1) % 4 - nbytes - col) % 4 + 4))
        else:
            e = _random_entry(rng, DECODE_MIXED_PATHS[blk] == "global")
        entries.append(e)
        nbytes += len(e[0])
    return _pack(entries)


def varint_edge_values():
    vals = [0, 1, 1 << 62, (1 << 63) - 1]
    for k in range(1, 9):
        vals += [(1 << (7 * k)) - 1, 1 << (7 * k)]
    return sorted(set(vals))


def decode_kat_batch():
    """Known answers: other and rel at the varint length edges in the three id layouts (MULTI backward /
    backward, unique forward / forward, constrained backward / forward), both directions; type counts
    at the header's prefix-varint lengths (2^3, 2^10, 2^17, 2^24, each -1, +0, +1) as edges and keys."""
    vals = varint_edge_values()
    entries = []
    for i, v in enumerate(vals):
        w = vals[(7 * i + 3) % len(vals)]
        for direction in (ec.OUT, ec.IN):
            entries.append(_edge(LABELS[0], direction, v, w))
            entries.append(_edge(LABELS[4], direction, v, w, ec.ONE2ONE))
            entries.append(_edge(LABELS[1], direction, v, w, ec.SIMPLE))
            entries.append(_edge(LABELS[1], direction, w, v, ec.SIMPLE, value=b"\x81"))
    for p in (3, 10, 17, 24):
        for count in ((1 << p) - 1, 1 << p, (1 << p) + 1):
            for direction in (ec.OUT, ec.IN):
                entries.append(_edge(ec.schema_id(count, "user_edge"), direction, 256, 9))
            entries.append(_prop(ec.schema_id(count, "user_key"), 9, b"v"))
            entries.append(_prop(ec.schema_id(count, "system_key"), 9, b"v"))
            b, vp = ec.encode_edge(ec.schema_id(count, "system_edge"), ec.OUT, 256, 9)
            entries.append((b, vp, (ec.schema_id(count, "system_edge"), 3, -1, -1)))
    return _pack(entries)


MALFORMED = -1
DECODE_MALFORMED_PATHS = ["staged", "global", "staged"]


def _malformed_parts():
    """The three malformed entries and the well-formed neighbours that would complete their varints."""
    bad = (0, MALFORMED, -1, -1)
    header = ec.write_relation_type(LABELS[4], True, ec.OUT)
    parts = {
        "no_stop": (bytes([0x70, 0x01, 0x02]), 3, bad),           # user edge, continuation bit, no stop byte
        "off_end": (header + b"\x01\x02", len(header), bad),      # ONE2ONE: ids forward from the value position
        "at_zero": (BAD_ENTRY, len(BAD_ENTRY), bad),              # MULTI: ids backward from the value position
        "stopper": _edge(LABELS[0], ec.IN, 0x33 << 8, 77, invisible=True),  # first byte >= 0x80
        "ender": _edge(LABELS[4], ec.OUT, 512, 5, ec.ONE2ONE),    # last byte: the stop byte of rel
    }
    assert parts["stopper"][0][0] & 0x80 and parts["no_stop"][0][0] & 0x10 and parts["ender"][0][-1] & 0x80
    return parts


def decode_malformed_batch():
    """Three blocks (staged, global, staged and partial).  Each holds the three malformed entries between
    well-formed ones: a header varint with no stop byte and a forward id that runs off the entry, each
    directly in front of an entry whose first byte is a stop byte (an invisible edge: 0xa0 | ...), and a
    backward id that reaches position 0, directly behind an entry whose last byte is a stop byte; block 0
    starts with the backward one (nothing in front of the array).  Expected: dir = other = rel = -1.
    Each malformed entry as the very last of an array: decode_malformed_last_batches."""
    rng = np.random.default_rng(32)
    m = _malformed_parts()
    entries = []
    for blk, path in enumerate(DECODE_MALFORMED_PATHS):
        n = DECODE_BLOCK if blk < 2 else 91
        block = [_random_entry(rng, path == "global") for _ in range(n)]
        for at, group in ((0, ["no_stop", "stopper"]), (40, ["off_end", "stopper"]), (80, ["ender", "at_zero"])):
            block[at:at + 2] = [m[k] for k in group]
        if blk == 0:
            block[0:2] = [m["at_zero"], m["ender"]]
        if blk == 2:
            block[-2:] = [m["no_stop"], m["off_end"]]
        entries += block
    return _pack(entries)


MALFORMED_LAST = [(kind, path) for kind in ("no_stop", "off_end", "at_zero") for path in ("staged", "global")]


def decode_malformed_last_batch(kind, path):
    """Two full blocks of well-formed entries whose very last entry is the malformed one of `kind`: what
    follows a header or forward varint without a stop byte is the byte array's padding (every byte a stop
    byte under JG_DEV_POISON=ff).  The backward one stands behind an entry ending in a stop byte.  path:
    the stage path of the last block (global: long values)."""
    rng = np.random.default_rng(33 + len(kind) + len(path))
    m = _malformed_parts()
    entries = [_random_entry(rng, False) for _ in range(DECODE_BLOCK)]
    entries += [_random_entry(rng, path == "global") for _ in range(DECODE_BLOCK)]
    entries[-2:] = [m["ender"], m[kind]]
    return _pack(entries)


def test_decode_batches_reach_their_paths(oracle_lib):
    data, off, vpos, want = decode_mixed_batch()
    assert decode_paths(off) == DECODE_MIXED_PATHS and (len(vpos) % DECODE_BLOCK) != 0
    assert [int(off[b]) % 4 for b in range(0, len(vpos), DECODE_BLOCK)][:8] == [0, 1, 2, 3, 0, 1, 2, 3]
    got = np.stack(oracle_lib.decode_edges(data, off, vpos, TIDS, TMULT), axis=1)
    np.testing.assert_array_equal(got, want)
    data, off, vpos, want = decode_kat_batch()
    got = np.stack(oracle_lib.decode_edges(data, off, vpos, TIDS, TMULT), axis=1)
    np.testing.assert_array_equal(got, want)
    data, off, vpos, want = decode_malformed_batch()
    assert decode_paths(off) == DECODE_MALFORMED_PATHS
    assert (want[:, 1] == MALFORMED).sum() == 3 * 3 + 2 and want[-1, 1] == MALFORMED
    assert np.all(np.diff(off) >= 1) and np.all(vpos >= 1) and np.all(vpos <= np.diff(off))  # check_entries
    for kind, path in MALFORMED_LAST:
        data, off, vpos, want = decode_malformed_last_batch(kind, path)
        assert decode_paths(off) == ["staged", path] and len(data) == off[-1]
        assert want[-1, 1] == MALFORMED and (want[:, 1] == MALFORMED).sum() == 1
        assert np.all(vpos >= 1) and np.all(vpos <= np.diff(off))  # check_entries
