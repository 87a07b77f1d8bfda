"""sampler._launch_schedule: the number and size of MCMCSampler.run's launches
as plain numbers, against values worked out by hand from the reference loop
(sampler.py:18-28) and the launch rules: at most `spl` steps per launch,
spl // interval samples per block-wise launch, segments that end where the
sample buffer is full or a copy block ends.  No GPU is used."""
from ip_mcmc_amd.sampler import _launch_schedule

BIG = 16384  # the default STEPS_PER_LAUNCH


def _rows(segments):
    return [tuple(s) for s in segments]


def test_blockwise_two_samples_per_launch():
    # spl 7, interval 3: two samples (6 steps) per launch; 5 samples = 2 such launches + one of 1 sample
    burn, segs = _launch_schedule(10, 5, 3, 7, 5, [5], True)
    assert burn == [7, 3]
    assert _rows(segs) == [(0, 0, 5, [(2, 6, 2), (1, 3, 1)], ())]


def test_per_sample_interval_above_launch_length():
    burn, segs = _launch_schedule(30, 9, 20, 7, 9, [9], False)
    assert burn == [7, 7, 7, 7, 2]
    assert len(segs) == 1 and segs[0][:4] == (0, 0, 9, ())
    assert [list(c) for c in segs[0][4]] == [[(7, False), (7, False), (6, True)]] * 9


def test_per_sample_exact_multiple_of_launch_length():
    _, segs = _launch_schedule(0, 2, 14, 7, 2, [2], False)
    assert [list(c) for c in segs[0][4]] == [[(7, False), (7, True)]] * 2


def test_interval_zero_records_the_current_state():
    burn, segs = _launch_schedule(6, 4, 0, BIG, 4, [4], False)
    assert burn == [6]
    assert _rows(segs) == [(0, 0, 4, (), [[(0, True)]] * 4)]


def test_streaming_segments_start_at_slot_zero():
    # 5 461 samples would fit one launch: each flush block is one launch of all its samples
    burn, segs = _launch_schedule(7, 23, 3, BIG, 5, [23], True)
    assert burn == [7]
    assert [s[:3] for s in segs] == [(0, 0, 5), (5, 0, 5), (10, 0, 5), (15, 0, 5), (20, 0, 3)]
    assert [s[3] for s in segs] == [[(1, 15, 5)]] * 4 + [[(1, 9, 3)]]
    # the per-sample loop (verbose) flushes at the same samples
    _, segs = _launch_schedule(7, 23, 3, BIG, 5, [23], False)
    assert [s[:3] for s in segs] == [(0, 0, 5), (5, 0, 5), (10, 0, 5), (15, 0, 5), (20, 0, 3)]
    assert all(list(c) == [(3, True)] for s in segs for c in s[4]) and sum(len(s[4]) for s in segs) == 23


def test_overlap_blocks_of_37_samples():
    bounds = [(j + 1) * 36 // 7 for j in range(7)] + [37]
    assert bounds == [5, 10, 15, 20, 25, 30, 36, 37]
    _, segs = _launch_schedule(3, 37, 4, BIG, 37, bounds, True)
    firsts = [0] + bounds[:-1]
    assert [s[0] for s in segs] == firsts and [s[1] for s in segs] == firsts
    assert [s[0] + s[2] for s in segs] == bounds
    assert [s[3] for s in segs] == [[(1, 4 * (b - a), b - a)] for a, b in zip(firsts, bounds)]
    # one sample per launch (spl 7 < 2 * 4): as many launches as samples, no remainder launch
    _, segs = _launch_schedule(3, 37, 4, 7, 37, bounds, True)
    assert [s[3] for s in segs] == [[(b - a, 4, 1)] for a, b in zip(firsts, bounds)]


def test_no_samples_and_no_burn_in():
    assert _launch_schedule(20, 0, 3, 7, 0, [0], True) == ([7, 7, 6], [])
    assert _launch_schedule(20, 0, 3, 7, 1, [0], False) == ([7, 7, 6], [])  # a streaming buffer is >= 1 sample
    burn, segs = _launch_schedule(0, 3, 2, 7, 3, [3], True)
    assert burn == [] and _rows(segs) == [(0, 0, 3, [(1, 6, 3)], ())]
    assert _launch_schedule(0, 0, 0, 7, 0, [0], False) == ([], [])


def test_steps_add_up():
    for n_burn, n, iv, spl, buf, blockwise in [(10, 5, 3, 7, 5, True), (33, 11, 5, 4, 3, False), (0, 7, 9, 2, 7, False),
                                               (5, 13, 2, 7, 4, True)]:
        burn, segs = _launch_schedule(n_burn, n, iv, spl, buf, [n], blockwise)
        steps = sum(nl * st for s in segs for nl, st, _ in s[3]) + sum(st for s in segs for c in s[4] for st, _ in c)
        assert sum(burn) == n_burn and steps == n * iv and sum(s[2] for s in segs) == n
        assert max(burn + [st for s in segs for _, st, _ in s[3]] + [0]) <= spl
