"""The job table of tests/_context_jobs.py on the CPU: it builds, every oracle expectation computes, and the set covers what the context
and thread tests rely on — a device job per family, both input forms, start tours, several runs per record size, a host-answered job
between device jobs, and a sequence in which every host path follows every other.  So the table cannot lose a family unnoticed."""
import _context_jobs as CJ


def test_the_table_covers_every_family_and_every_ordered_pair():
    table = CJ.jobs()
    want = [j.oracle() for j in table]
    assert all(w is not None and w == j.oracle() for j, w in zip(table[:2], want))  # (an expectation is a pure function of the job)
    CJ.check_coverage(table)
    assert len({j.name for j in table}) == len(table)
    assert {j.family for j in table} == set(CJ.FAMILIES) == {f for fs in CJ.GROUPS.values() for f in fs} and len(CJ.FAMILIES) == 17
    assert sum(j.matrix for j in table) >= 5 and sum(j.init for j in table) >= 4
    assert sum(3 <= j.count <= 8 and j.record == 16 for j in table) >= 1 and sum(3 <= j.count <= 8 and j.record == 32 for j in table) >= 1
    reps = CJ.representatives(table)
    assert len(reps) == len(CJ.GROUPS) == 10 and len(CJ.euler_sequence(10)) == 91
    for g in (2, 3, 4, 7):
        seq = CJ.euler_sequence(g)
        assert seq[0] == seq[-1] and sorted(zip(seq, seq[1:])) == [(a, b) for a in range(g) for b in range(g) if a != b]
    # every expectation holds a tour of its own n (the host jobs: n = 1 and 2), so a job cannot pass by comparing nothing
    for j, w in zip(table, want):
        first = w[0][0] if isinstance(w[0][0], list) else w[0]
        assert len(first) >= 1 and (len(first) == j.size or "(host)" in j.name), j.name
