"""GPU tests of what the view-graph operations share (csrc/sfm_view_graph.h) and the three suites of its callers do not pin:
the device check of the rotations in the ``_dev`` forms.  One kernel of 256 threads and one word serve the three calls; the
sizes 255 and 257 put the last matrix at the end of the first workgroup and alone in the second.

What else the header shares is pinned where it was: depths in global memory by ``test_gpu_rotavg.test_depths_in_global_memory``
(4 100 views), the second chunk of ``block_dot`` by the case ``size_1100_2049`` of tests/_transavg_reference.py, the levels and
the roots without an edge by the ``two_components`` / ``root_masked`` cases of both averaging suites."""
import numpy as np
import pytest

import _rotavg_reference as rr
import _transavg_reference as tr
from _twoview_checks import same_bits

pytestmark = pytest.mark.gpu

SIZES = (255, 257)


def bad_sets(n):
    """Index 0 only, the last index only, two at once (the lower one is to be named)."""
    return ((0,), (n - 1,), (n - 1, n // 2))


def stretched(M, rows):
    M = M.copy()
    M[list(rows)] *= 1.01                                     # det = 1.01^3: verify_rotation refuses it
    return M


@pytest.fixture(scope="module")
def edge_graph():
    """70 views, E edges with their relative rotations, for E in SIZES."""
    return {E: rr.make_case("edges_%d" % E, 70, rr.topo_random(70, np.random.default_rng(E), E), E, max_hyp=2, iters=1, steps=1)
            for E in SIZES}


@pytest.fixture(scope="module")
def view_graph():
    """V views with their rotations and 2 V edges, for V in SIZES."""
    return {V: tr.make_case("views_%d" % V, V, rr.topo_random(V, np.random.default_rng(V), 2 * V), V, rounds=1) for V in SIZES}


@pytest.mark.parametrize("E", SIZES)
def test_rotation_average_dev_names_the_lowest_bad_edge(hip, edge_graph, E):
    import torch
    c = edge_graph[E]
    d_R = torch.full((c.V, 9), 7.0, dtype=torch.float64, device="cuda")
    for rows in bad_sets(E):
        d_rel = torch.from_numpy(stretched(c.rel, rows)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="Rel of edge %d is not a rotation" % min(rows)):
            hip.rotation_average_dev(c.V, c.edges, d_rel.data_ptr(), root=0, cos_max=c.cos_max, max_hyp=2, iters=1, steps=1,
                                     d_R_out=d_R.data_ptr())
    assert np.all(d_R.cpu().numpy() == 7.0)                   # nothing else was launched


@pytest.mark.parametrize("E", SIZES)
def test_view_triplets_dev_names_the_lowest_bad_edge(hip, edge_graph, E):
    import torch
    c = edge_graph[E]
    d_keep = torch.full((E,), 7, dtype=torch.uint8, device="cuda")
    for rows in bad_sets(E):
        d_rel = torch.from_numpy(stretched(c.rel, rows)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="Rel of edge %d is not a rotation" % min(rows)):
            hip.view_triplets_dev(c.V, c.edges, d_rel.data_ptr(), cos_loop=c.cos_max, d_edge_keep=d_keep.data_ptr())
    assert np.all(d_keep.cpu().numpy() == 7)


@pytest.mark.parametrize("V", SIZES)
def test_translation_average_dev_names_the_lowest_bad_view(hip, view_graph, V):
    import torch
    c = view_graph[V]
    d_t = torch.from_numpy(c.t).cuda()
    d_C = torch.full((V, 3), 7.0, dtype=torch.float64, device="cuda")
    for rows in bad_sets(V):
        R = stretched(c.R, rows)
        R[1] = 0.0                                            # nine zeros below a bad view (or above view 0): never the one named
        d_Rv = torch.from_numpy(R).cuda()
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="R of view %d is not a rotation" % min(rows)):
            hip.translation_average_dev(V, c.edges, d_Rv.data_ptr(), d_t.data_ptr(), root=0, cos_max=c.cos_max, rounds=1,
                                        d_C_out=d_C.data_ptr())
    assert np.all(d_C.cpu().numpy() == 7.0)


@pytest.mark.parametrize("V", SIZES)
def test_translation_average_dev_skips_views_without_rotation(hip, view_graph, V):
    """Nine zeros are "no rotation", not a bad one: the ``_dev`` form goes through and gives the bits of the host form."""
    import torch
    c = view_graph[V]
    R = c.R.copy()
    R[[1, V // 2, V - 1]] = 0.0
    kw = dict(root=0, cos_max=c.cos_max, mu=c.mu, rounds=1, polish=1, cg_tol=c.cg_tol, cg_max=c.cg_max)
    host = hip.translation_average(V, c.edges, R, c.t, outputs=("view_status", "status"), **kw)
    assert np.array_equal(np.flatnonzero(host[4] & hip.TRANSAVG_NO_ROTATION), [1, V // 2, V - 1]) and not host[6] & hip.TRANSAVG_NO_MODEL
    d_Rv, d_t = torch.from_numpy(R).cuda(), torch.from_numpy(c.t).cuda()
    d_C = torch.zeros((V, 3), dtype=torch.float64, device="cuda")
    d_view = torch.zeros(V, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hip.translation_average_dev(V, c.edges, d_Rv.data_ptr(), d_t.data_ptr(), d_C_out=d_C.data_ptr(), d_view_status=d_view.data_ptr(), **kw)
    assert same_bits(d_C.cpu().numpy(), host[0]) and same_bits(d_view.cpu().numpy(), host[4])
