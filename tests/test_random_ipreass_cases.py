"""What the seeded scenarios of ipreass_cases.py cover, from the models alone (no GPU): every
per-frame and per-datagram verdict and every incompleteness cause occur, at least a third of the
groups are complete and at least a third incomplete; and in every scenario the hole algorithm
completes every group the declarative model completes."""
import collections

import ipreass_cases as R


def test_the_scenarios_cover_every_verdict_and_cause(oracle):
    frame_v, dgram_v, causes = collections.Counter(), collections.Counter(), collections.Counter()
    complete = incomplete = 0
    for seed in R.SEEDS:
        s = R.scenario(oracle, seed)
        e = R.model(oracle, s.batch, s.max_reass)
        frame_v.update(e.verdict.tolist())
        for key, order in e.complete.items():
            dgram_v[int(e.dgram[order[0]]["verdict"])] += 1
        complete += len(e.complete)
        incomplete += len(e.groups) - len(e.complete)
        for key, cause in s.causes.items():
            assert key not in e.complete, (seed, key, cause)
            causes[cause] += 1
        hole = R.feed_batch(s.batch, e, s.max_reass)
        for key, order in e.complete.items():
            assert [(i, b) for i, b in hole.get(key, [])] == [(max(order), e.body[key])], (seed, key)
    assert set(frame_v) == {0, 1, 2, 3, 4, 5, 6, 7, 8, 14, 15}, frame_v
    assert set(dgram_v) == {R.ACCEPT, R.NO_CHKSUM, R.OTHER, R.L4_MALFORMED, R.L4_CHKSUM, R.TRUNCATED}, dgram_v
    assert set(causes) == set(R.CAUSES) and min(causes.values()) >= 5, causes
    total = complete + incomplete
    assert total >= 800 and 3 * complete >= total and 3 * incomplete >= total, (complete, incomplete)
