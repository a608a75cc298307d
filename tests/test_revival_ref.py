"""The truth of tests/revival_cases.py, checked from the Python cache mirror
alone (no library): which rounds a resident session must refuse because a
queue or job name returns with what the cache kept for it, and that every
such round would go wrong if it were applied naively."""
import pytest

from revival_cases import CALLER_ONLY, CASES, EXPECT, GPU_SEEDS, SEEDS, fuzz_fixture, fuzz_rounds, refused_name, verdicts


def test_every_case_has_its_verdict_written_out():
    assert sorted(CASES) == sorted(EXPECT)
    accept = sorted(c for c in EXPECT if EXPECT[c] is None)
    assert accept == ["empty_pod_group_back", "empty_pod_group_back_same_batch", "jobless_queue_back",
                      "jobless_queue_back_same_batch", "jobless_queue_updated_back"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_case_verdict(case):
    fx0, rounds = CASES[case]()
    want = verdicts(fx0, rounds)
    if EXPECT[case] is None:
        assert want == [None] * len(rounds)
        return
    r, name = EXPECT[case]
    assert r == len(rounds) - 1  # the refused round is the case's last
    assert want[:r] == [None] * r and want[r] is not None
    v = want[r]
    assert (v.round, refused_name(v)) == (r, name)
    assert v.seen == (case not in CALLER_ONLY)
    # otherwise the case proves nothing: applied naively, the session lacks a job or a job's tasks
    assert v.differs and (v.naive_jobs != v.jobs or v.naive_tasks != v.tasks)
    assert v.tasks > 0 or v.job not in v.naive_jobs


def test_the_two_recorded_failures():
    """What a session that takes the batches holds against the reference's cache."""
    fx0, rounds = CASES["queue_same_batch"]()
    v = verdicts(fx0, rounds)[0]
    assert (v.rule, v.naive_jobs, sorted(v.jobs)) == ("a", ["qb/pgb"], ["qa/pga", "qb/pgb"])
    fx0, rounds = CASES["pod_group_same_batch"]()
    v = verdicts(fx0, rounds)[0]
    assert (v.rule, v.job, v.naive_tasks, v.tasks) == ("b", "qa/pga", 0, 4)


def test_generated_seeds_cover_both_directions():
    refused = accepted = 0
    same_batch = later = 0
    for seed in SEEDS:
        fx0 = fuzz_fixture(seed)
        rounds = fuzz_rounds(fx0, seed)
        assert 1 <= len(rounds) <= 3
        want = verdicts(fx0, rounds)
        assert len(want) == len(rounds)  # a refused round is the last one generated
        if want[-1] is None:
            accepted += 1
            continue
        refused += 1
        v = want[-1]
        assert v.differs, seed
        assert v.seen, seed  # the generator only returns names that left
        if v.round == 0:
            same_batch += 1
        else:
            later += 1
    assert len(SEEDS) >= 36 and len(set(SEEDS)) == len(SEEDS)
    assert 3 * refused >= len(SEEDS) and 3 * accepted >= len(SEEDS)
    assert same_batch >= 3 and later >= 3  # in the batch that deleted the name, and in a later update
    assert len(GPU_SEEDS) == 6 and set(GPU_SEEDS) <= set(SEEDS)
    ends = [verdicts(fuzz_fixture(s), fuzz_rounds(fuzz_fixture(s), s))[-1] for s in GPU_SEEDS]
    assert sum(1 for v in ends if v is None) >= 2 and sum(1 for v in ends if v is not None) >= 2
