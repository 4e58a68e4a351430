"""CPU checks of the graph observations' host side (npp_graph.cpp behind npp_graph_compile) against tests/golden/graph.npz: the
node features, edge index and counts that the reference's GraphBuilder.build_graph + create_graph_data produce on the LevelData
of the env's reset (tests/golden/make_golden_graph.py), for the door, mine, curriculum-0, zoo and official levels, a level with
two exits and an open level past the node and edge limits.  Compared bit for bit, padding included."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def graph():
    from nclone_amd import build_native

    build_native.build()
    z = np.load(os.path.join(ROOT, "tests", "golden", "graph.npz"))
    return z, bytes(z["names"]).decode().split("\n")


def test_fixture_covers_the_cases(graph):
    z, names = graph
    kinds = {n.split(":")[0] for n in names}
    assert {"doors", "mines", "c0", "zoo", "official", "crafted"} <= kinds
    assert sum(n.startswith("official:") for n in names) == 5
    feats = np.concatenate([z["f%d" % k] for k in range(len(names))])
    rows = {tuple(r) for r in feats[:, 2:].tolist()}
    assert {(-1.0, np.float32(0.2), 1.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, 1.0)} <= rows   # mines, exits, locked doors
    k = names.index("crafted:open")
    assert int(z["nn%d" % k]) == 2500 and int(z["ne%d" % k]) > 19000   # node list truncated, edges into it skipped


def _compare_graph_rows(z, names):
    from nclone_amd.engine import graph_tables

    for k, name in enumerate(names):
        feats, edges, nn, ne = graph_tables(z["m%d" % k])
        assert (nn, ne) == (int(z["nn%d" % k]), int(z["ne%d" % k])), name
        assert feats.tobytes()[: nn * 24] == z["f%d" % k].tobytes(), name
        assert not feats[nn:].any(), name
        assert np.array_equal(edges[:, :ne], z["e%d" % k]), name
        assert not edges[:, ne:].any(), name


def test_graph_compile_matches_reference(graph):
    _compare_graph_rows(*graph)


def test_graph_compile_matches_reference_on_test_maps():
    """graph2.npz (make_golden_graph.py 2): the reference's 16 held-out test maps -- locked doors, a trap door and one-way
    platforms, 29 toggle mines, four open maps past the 2500-node limit, a map without entities."""
    from nclone_amd import build_native

    build_native.build()
    z = np.load(os.path.join(ROOT, "tests", "golden", "graph2.npz"))
    names = bytes(z["names"]).decode().split("\n")
    assert len(names) == 16 and all(n.startswith("test_maps:") for n in names)
    assert sum(int(z["nn%d" % k]) == 2500 for k in range(16)) == 4
    _compare_graph_rows(z, names)


def test_several_exits_and_empty_adjacency():
    """A level with two exits gets a graph (npp_reachability refuses it); a level whose spawn is walled in has no edge at all:
    the reference's create_graph_data then makes one node at (0, 0)."""
    from nclone_amd.engine import graph_tables, reach_level_info

    z = np.load(os.path.join(ROOT, "tests", "golden", "graph.npz"))
    names = bytes(z["names"]).decode().split("\n")
    two = z["m%d" % names.index("crafted:two_exits")]
    assert not reach_level_info(two)["supported"]
    assert graph_tables(two)[3] > 0
    solid = np.array(two, copy=True)
    solid[184:184 + 966] = 1
    feats, edges, nn, ne = graph_tables(solid)
    assert (nn, ne) == (1, 0)
    assert not feats.any() and not edges.any()
