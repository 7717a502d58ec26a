"""CPU tests of the mutation corpus (tests/rdbload_mutants.py) under tests/rdbload_reference.py:
that it is deterministic and large, that it reaches every status often enough for the GPU sweep
(tests/test_gpu_rdbload_edges.py) to mean something, and the two properties the GPU tests lean on:
the bound, and that every strict prefix of a seed is RR_RDBLOAD_E_TRUNC."""
import collections

import redrock_old_amd as rr

import lzf_reference as lzf
import rdbload_mutants as mu
import rdbload_reference as ld


def results():
    types, pays, origin = mu.corpus()
    return types, pays, origin, [ld.load_blob(t, p, mu.OPTS) for t, p in zip(types, pays)]


def test_seeds_are_valid_or_convert():
    st = [ld.load_blob(t, p, mu.OPTS)[0] for t, p in mu.seeds()]
    assert set(st) == {0, ld.E_CONVERT}
    assert st.count(0) >= 5 and st.count(ld.E_CONVERT) >= 4            # corruptions cross the thresholds both ways
    kinds = {t for t, _ in mu.seeds()}
    assert kinds == set(ld.TYPES)
    lens = [len(p) for _, p in mu.seeds()]
    assert max(lens) < 400 and sum(lens) < 1200


def test_corpus_is_deterministic_and_large():
    a, b = mu.corpus(), mu.corpus()
    assert a == b
    assert len(a[0]) == len(a[1]) == len(a[2]) >= 10000
    assert sum(len(p) for p in a[1]) < 8 << 20


def test_corpus_reaches_every_status():
    types, pays, origin, res = results()
    count = collections.Counter(r[0] for r in res)
    print(sorted(count.items()))
    assert set(count) == {0, 32, 33, 34, 35, 36, 37, 38}
    for st in range(33, 39):
        assert count[st] >= 100, (st, count[st])
    # the precedences the header states, each met by some mutant: a value whose walk fails although
    # bytes are left over or a conversion is due gets the walk's status (the first defect decides)
    by_seed = collections.defaultdict(set)
    for (si, kind, pos), r in zip(origin, res):
        by_seed[si].add(r[0])
    seed_st = [ld.load_blob(t, p, mu.OPTS)[0] for t, p in mu.seeds()]
    for si, st in enumerate(seed_st):
        if st == ld.E_CONVERT:                                             # a CONVERT seed also yields the earlier statuses
            assert {ld.E_TRUNC, ld.E_EXTRA} <= by_seed[si], (si, by_seed[si])


def test_blobs_stay_within_the_bound(monkeypatch):
    """rr_rdbload_bound holds for every mutant that loads and met no LZF string."""
    calls = []
    real = lzf.decompress
    monkeypatch.setattr(lzf, "decompress", lambda s, n: (calls.append(1), real(s, n))[1])
    types, pays, _ = mu.corpus()
    checked = 0
    for t, p in zip(types, pays):
        del calls[:]
        st, blob, _, _ = ld.load_blob(t, p, mu.OPTS)
        if st == 0 and not calls:
            assert len(blob) <= rr.rdbload_bound(1, len(p)), (t, p)
            checked += 1
    assert checked >= 3000


def test_every_strict_prefix_of_a_seed_is_trunc():
    n = 0
    for t, p in mu.seeds():
        for k in range(len(p)):
            assert ld.load_blob(t, p[:k], mu.OPTS)[0] == ld.E_TRUNC, (t, p, k)
            n += 1
    assert n >= 500
