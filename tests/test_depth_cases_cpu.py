"""The conditions the depth-sweep inputs are there for (depth_cases), on the models alone: the answer moves with the depth
on the fixtures the project already has — else the GPU tests would compare equal things."""
import pcr_run_cases as cases
import pcr_run_ref as ref

import depth_cases as dc


def test_18s_appears_at_depth_two(orc):
    first = dc.expected_18s(orc, 1)
    assert first.status == ref.NO_PRIMERS and not first.products
    for d in range(2, dc.CHUNKS_18S + 1):
        o = dc.expected_18s(orc, d)
        assert o.status == ref.SUCCESS and len(o.products) == 1, d


def test_mixed_panel_moves_with_depth(orc):
    status = {d: [o.status for o in dc.mixed_expected(orc, d)] for d in range(1, dc.CHUNKS_MIXED + 1)}
    assert status[1] != status[2] and status[2] != status[3] and status[1] != status[3]
    assert sum(s == ref.SUCCESS for s in status[2]) >= 2
    assert sum(s == ref.SUCCESS for s in status[3]) >= 7
    # the last depth is the merged table: what shk_pcr_run's own tests expect
    full, want = dc.mixed_expected(orc, dc.CHUNKS_MIXED), cases.mixed_expected(orc, "none")
    assert [(o.status, o.n_nodes, o.n_edges, o.threshold_used, [r.sequence for r in o.products]) for o in full] == \
           [(o.status, o.n_nodes, o.n_edges, o.threshold_used, [r.sequence for r in o.products]) for o in want]


def test_chunk_bases_add_up(orc):
    import pcr_panel_cases as pc
    p = pc.mixed_panel(orc)
    per = dc.chunk_bases(orc, p.bases, p.offsets, p.k, dc.CHUNKS_MIXED)
    assert sum(per) == int(orc.run_batch(p.bases, p.offsets, p.k, 1, 100).stats["n_bases_ingested"])
