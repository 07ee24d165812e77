"""check_rows of tests/test_gpu_build_edges.py can fail: a correct read-back made in numpy passes, and each way a
CSR build can go wrong at a tile edge (an order, a row boundary, a lost or doubled entry, a split run) raises.  No GPU."""
import numpy as np
import pytest

from test_gpu_build_edges import DIR_BOTH, DIR_IN, DIR_OUT, check_rows, numpy_rows, tile_graph

N = 40
DIRS = [DIR_OUT, DIR_IN, DIR_BOTH]


@pytest.fixture(scope="module")
def edges():
    """2100 edges over 40 vertices with tile_graph's seeding: self-loops, a run of one pair, its reverse, ghosts."""
    el = tile_graph(N, 2100)
    run = np.flatnonzero((el.si == el.si[10]) & (el.di == el.di[10]))
    assert el.si[10] != el.di[10] and len(run) >= 3 and (el.si[el.real] == el.di[el.real]).sum() >= 2
    assert len(el.real) < el.m  # ghosts are there
    return el


def rows_of(el, direction):
    off, nbr, edge = numpy_rows(N, el.si, el.di, direction)
    return off.copy(), nbr.copy(), edge.copy()


def run_of_the_pair(el, direction, off, nbr):
    """Entry positions of the seeded pair's run in the row that holds it under `direction`."""
    a, b = int(el.si[10]), int(el.di[10])
    owner, other = (b, a) if direction == DIR_IN else (a, b)
    at = off[owner] + np.flatnonzero(nbr[off[owner]:off[owner + 1]] == other)
    assert len(at) >= 3 and (np.diff(at) == 1).all()
    return at


@pytest.mark.parametrize("direction", DIRS)
def test_a_correct_read_back_passes(edges, direction):
    off, nbr, edge = rows_of(edges, direction)
    check_rows(N, edges.si, edges.di, direction, off, nbr, edge)
    check_rows(N, edges.si, edges.di, direction, off, nbr)  # and without ordinals
    empty = np.zeros(0, np.int64)
    check_rows(N, empty, empty, direction, np.zeros(N + 1, np.int64), empty, empty.astype(np.uint32))


@pytest.mark.parametrize("direction", DIRS)
def test_two_ordinals_swapped_inside_a_run(edges, direction):
    off, nbr, edge = rows_of(edges, direction)
    at = run_of_the_pair(edges, direction, off, nbr)
    edge[[at[0], at[1]]] = edge[[at[1], at[0]]]
    assert edge[at[0]] != edge[at[1]]
    with pytest.raises(AssertionError, match="ascend"):
        check_rows(N, edges.si, edges.di, direction, off, nbr, edge)
    check_rows(N, edges.si, edges.di, direction, off, nbr)  # invisible without ordinals: the pairs are the same


def test_a_self_loops_entries_parted(edges):
    """BOTH: a vertex with two self-loops lists [e, e, f, f]; [e, f, e, f] keeps the multiset and ascends weakly."""
    off, nbr, edge = rows_of(edges, DIR_BOTH)
    c = int(edges.si[3])
    at = off[c] + np.flatnonzero(nbr[off[c]:off[c + 1]] == c)
    assert len(at) >= 4 and edge[at[0]] == edge[at[1]] < edge[at[2]] == edge[at[3]]
    edge[[at[1], at[2]]] = edge[[at[2], at[1]]]
    with pytest.raises(AssertionError, match="self-loop"):
        check_rows(N, edges.si, edges.di, DIR_BOTH, off, nbr, edge)


@pytest.mark.parametrize("with_ordinals", [True, False])
@pytest.mark.parametrize("direction", DIRS)
def test_an_entry_moved_to_the_neighbouring_row(edges, direction, with_ordinals):
    off, nbr, edge = rows_of(edges, direction)
    r = next(r for r in range(N - 1) if off[r + 1] > off[r] and nbr[off[r + 1] - 1] != r)
    off[r + 1] -= 1  # row r's last entry now opens row r + 1
    with pytest.raises(AssertionError):
        check_rows(N, edges.si, edges.di, direction, off, nbr, edge if with_ordinals else None)


@pytest.mark.parametrize("with_ordinals", [True, False])
@pytest.mark.parametrize("direction", DIRS)
def test_an_entry_dropped_or_duplicated(edges, direction, with_ordinals):
    off, nbr, edge = rows_of(edges, direction)
    r = int(np.argmax(np.diff(off)))
    k = off[r]
    for delta in (-1, 1):  # dropped; duplicated in place
        nbr2 = np.delete(nbr, k) if delta < 0 else np.insert(nbr, k, nbr[k])
        edge2 = np.delete(edge, k) if delta < 0 else np.insert(edge, k, edge[k])
        off2 = off.copy()
        off2[r + 1:] += delta
        with pytest.raises(AssertionError, match="kept edges"):
            check_rows(N, edges.si, edges.di, direction, off2, nbr2, edge2 if with_ordinals else None)


@pytest.mark.parametrize("with_ordinals", [True, False])
@pytest.mark.parametrize("direction", DIRS)
def test_one_entry_lost_and_another_doubled(edges, direction, with_ordinals):
    """The counts stay right: only the pairs / the multiset of ordinals show it."""
    off, nbr, edge = rows_of(edges, direction)
    r = next(r for r in range(N) if off[r + 1] - off[r] >= 2 and nbr[off[r]] != nbr[off[r] + 1])
    nbr[off[r] + 1], edge[off[r] + 1] = nbr[off[r]], edge[off[r]]
    with pytest.raises(AssertionError):
        check_rows(N, edges.si, edges.di, direction, off, nbr, edge if with_ordinals else None)


@pytest.mark.parametrize("direction", DIRS)
def test_only_an_ordinal_doubled(edges, direction):
    """Parallel edges: the second entry of the run repeats the first one's ordinal.  Every entry is still a true
    edge of its row and the pairs are unchanged; the multiset is not."""
    off, nbr, edge = rows_of(edges, direction)
    at = run_of_the_pair(edges, direction, off, nbr)
    edge[at[1]] = edge[at[0]]
    with pytest.raises(AssertionError, match="multiset"):
        check_rows(N, edges.si, edges.di, direction, off, nbr, edge)


@pytest.mark.parametrize("with_ordinals", [True, False])
@pytest.mark.parametrize("direction", DIRS)
def test_a_run_split_by_a_foreign_entry(edges, direction, with_ordinals):
    off, nbr, edge = rows_of(edges, direction)
    at = run_of_the_pair(edges, direction, off, nbr)
    a, b = int(edges.si[10]), int(edges.di[10])
    owner = b if direction == DIR_IN else a
    lo, hi = off[owner], off[owner + 1]
    foreign = next(k for k in range(lo, hi) if nbr[k] != nbr[at[0]])
    # an inner entry of the run and the foreign one change places: [x, x, x, .., y] -> [x, y, x, .., x]
    for arr in (nbr, edge):
        arr[[at[1], foreign]] = arr[[foreign, at[1]]]
    with pytest.raises(AssertionError, match="contiguous"):
        check_rows(N, edges.si, edges.di, direction, off, nbr, edge if with_ordinals else None)


def test_both_entries_of_an_edge_in_one_end_row(edges):
    """BOTH: edge a -> b listed twice in a's row and never in b's, its reverse b -> a twice in b's row: every entry
    is a true edge of its row, the pairs and the multiset hold, only the end rows tell."""
    si, di = np.asarray([0, 1, 2]), np.asarray([1, 0, 2])
    off, nbr, edge = numpy_rows(3, si, di, DIR_BOTH)
    check_rows(3, si, di, DIR_BOTH, off, nbr, edge)
    assert edge.tolist() == [0, 1, 0, 1, 2, 2]
    edge[:4] = [0, 0, 1, 1]
    with pytest.raises(AssertionError, match="end"):
        check_rows(3, si, di, DIR_BOTH, off, nbr, edge)


@pytest.mark.parametrize("direction", DIRS)
def test_off_not_monotone_or_short(edges, direction):
    off, nbr, edge = rows_of(edges, direction)
    bad = off.copy()
    r = int(np.argmax(np.diff(off)))
    bad[r + 1], bad[r] = off[r], off[r + 1]
    with pytest.raises(AssertionError, match="monotone"):
        check_rows(N, edges.si, edges.di, direction, bad, nbr, edge)
    with pytest.raises(AssertionError, match="monotone"):
        check_rows(N, edges.si, edges.di, direction, off[:-1], nbr, edge)
