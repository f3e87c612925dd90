"""CPU checks of tests/pcr_panel_cases.py: every panel has, by the model (tests/pcr_ref.py), the property it was built
for — so a GPU comparison on one of them is a comparison at that shape, and a case cannot quietly lose it.  No GPU."""
import pcr_panel_cases as pc
import pcr_ref as ref


def test_mixed_panel_ends_its_sweeps_in_every_way(orc):
    p = pc.mixed_panel(orc)
    assert p.k == 21 and len(p.genes) >= 8 and len(p.sets) == 2 * len(p.genes) == 2 * len(p.expected)
    by = {g.name: (g, p.sets[2 * i], p.sets[2 * i + 1]) + p.expected[i] for i, g in enumerate(p.genes)}

    def thresholds(name):
        g, f, r = by[name][:3]
        return ref.compute_coverage_thresholds(min(max(f[1], default=0), max(r[1], default=0)), g.params["min_count"])

    # found at the first threshold of a sweep that has more
    g, f, r, graph, used, steps = by["first threshold"]
    assert g.params["sweep"] and len(thresholds("first threshold")) > 1
    assert graph.found_path and steps == 1 and used == thresholds("first threshold")[0]
    # found only at a later step
    for name, at in (("second step", 2), ("third step", 3)):
        g, f, r, graph, used, steps = by[name]
        assert graph.found_path and steps == at and used == thresholds(name)[at - 1] and not graph.budget_break
    # never found: every step run, the last at min_count, no budget in the way
    g, f, r, graph, used, steps = by["never found"]
    assert len(f[0]) and len(r[0]) and not graph.found_path and not graph.budget_break
    assert steps == len(thresholds("never found")) > 1 and used == g.params["min_count"]
    assert len(graph.sub_kmer) > pc.MIXED_BUDGET  # (the budget of the others would have cut it)
    # stops on max_num_nodes
    g, f, r, graph, used, steps = by["budget"]
    assert g.params["max_num_nodes"] == pc.MIXED_BUDGET == 2500 and graph.budget_break
    assert len(graph.sub_kmer) == pc.MIXED_BUDGET + 1 and not graph.found_path
    # an empty forward set; both sets empty
    g, f, r, graph, used, steps = by["no forward set"]
    assert len(f[0]) == 0 and len(r[0]) > 0 and not graph.found_path and len(graph.sub_kmer) > len(r[0])
    g, f, r, graph, used, steps = by["no set at all"]
    assert len(f[0]) == 0 and len(r[0]) == 0 and len(graph.sub_kmer) == 0 and steps == 1
    # two genes with identical primers, not next to each other
    a, b = pc.gene_index(p, "twin a"), pc.gene_index(p, "twin b")
    assert abs(a - b) > 1 and p.genes[a][1:] == p.genes[b][1:]
    assert p.expected[a][0].sub_kmer == p.expected[b][0].sub_kmer and p.expected[a][0].edges == p.expected[b][0].edges
    assert p.expected[a][0].found_path and len(p.expected[a][0].sub_kmer) > 800
    # parameters differ along the panel
    assert len({tuple(sorted(g.params.items())) for g in p.genes}) >= 4
    assert not by["no sweep, ratio 1.5"][0].params["sweep"] and by["no sweep, ratio 1.5"][5] == 1


def test_wide_and_narrow_jobs_share_a_table():
    p = pc.wide_narrow_panel()
    widest = []
    for nodes, dirs, mc in p.jobs:
        widest.append(max(len(e) for e, _ in ref.neighborhood_levels(nodes, dirs, p.table, p.k, mc)))
    assert any(w > 1024 for w in widest) and any(w <= 1024 for w in widest), widest
    by = dict(zip(p.names, widest))
    assert by["flat1025"] > 1024 and by["rising"] > 1024 and by["falling"] > 1024  # wide at level 0, later, and at first only
    assert by["flat1025, 40 chains"] <= 1024 and by["rising, one chain"] <= 1024
    first = [len(ref.neighborhood_levels(n, d, p.table, p.k, mc)[0][0]) for n, d, mc in p.jobs]
    assert first[p.names.index("rising")] <= 1024 < first[p.names.index("falling")]


def test_many_jobs_are_distinct_and_more_than_the_card_holds(orc):
    p = pc.many_jobs_panel(orc)
    assert len(p.jobs) == 600 > 512 and p.k == 9
    seen = set()
    for nodes, dirs, mc in p.jobs:
        for n, d in zip(nodes, dirs):
            for b in (1, 2):
                if d & b:
                    assert (n, b) not in seen
                    seen.add((n, b))
    assert all(a[2] != b[2] for a, b in zip(p.jobs, p.jobs[1:]))
    # a few levels each: most jobs are still going when max_levels stops them, and they are not all alike
    outs = [ref.neighborhood(n, d, p.table, p.k, mc, max_levels=p.max_levels) for n, d, mc in p.jobs[:60]]
    assert sum(o[4] == p.max_levels for o in outs) > 30 and len({len(o[0]) for o in outs}) > 10
