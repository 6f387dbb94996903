"""CPU companions of tests/test_hstu_decode_kernel_gpu.py (the HSTU cached-decode kernel on every route and at its limits).

- The case table reaches the routes it claims, by the kernel's own formulas restated in tests/_hstu_decode_cases.py.
- Sensitivity: for every case and scenario the float64 restatement with each applicable mistake of R.BUGS and R.GEMV_BUGS injected lies
  outside the bar the GPU test holds the kernel to, on the current embeddings or on a cache row the decode writes.
- Limits: rails_hstu_decode_supported equals the restated LDS bound on a grid that holds both sides of every limit."""
import itertools
import os

import pytest
import torch

from tests import _hstu_cache_ref as R
from tests import _hstu_decode_cases as K

# ts_p (the query's timestamp read at p instead of min(p + 1, N - 1)) cannot show where both timestamps are equal in every row
TS_P_BLIND = {("scalar_w198", "equal", "tail"), ("scalar_w198", "equal", "interior")}


def applicable(name, kind, scen, bug):
    if bug == "return_p" and scen == "tail":              # the delta row IS the row at lengths - 1
        return False
    if bug == "ts_p" and not K.CASES[name].rel_bias:      # no timestamps enter the arithmetic
        return False
    if bug == "ts_p" and (name, kind, scen) in TS_P_BLIND:
        return False
    return True


def test_case_table_reaches_the_routes_it_names():
    for name, c in K.CASES.items():
        assert K.supported(c.N, c.D, c.H, c.dqk, c.dv, c.buckets), name
        assert K.route(c.W) == K.ROUTES[name], (name, c.W, K.route(c.W))
    assert K.route(256, aligned=False) == ("per-column", 0)
    c = K.CASES["scalar_w30"]
    assert c.D % 8 == 0                                   # no k remainder
    c = K.CASES["scalar_w198"]
    assert c.D % 8 == 2 and c.N - 1 > 64
    c = K.CASES["heads9"]
    S = K.ROUTES["heads9"][1]
    assert (c.W // 4) * S == 504 and c.D < 4 * S and c.D % S and c.H > 8 and c.buckets == 255
    c = K.CASES["b600"]
    assert K.ROUTES["b600"][1] > c.D and c.B > K.THREADS
    c = K.CASES["lds_limit"]
    assert K.BOUNDARY_PAIRS["H"][0] == (c.N, c.D, c.H, c.dqk, c.dv, c.buckets)
    assert not K.supported(c.N, c.D, c.H + 1, c.dqk, c.dv, c.buckets)
    assert K.CASES["d1024"].D == K.MAX_DIM > K.THREADS
    for name in K.CASES:                                   # the batches hold what the cases promise
        for scen in K.SCENARIOS:
            b = K.batch(name, "random", scen)
            c = K.CASES[name]
            assert int(b.lengths[0]) == c.N and int(b.lengths[1]) == 1 and bool(((b.positions >= 0) & (b.positions < b.lengths)).all())
            assert c.B < 3 or int(b.new_ids[2, b.positions[2]]) == 0
            assert scen == "tail" or bool((b.positions < b.lengths - 1).any())


def test_ts_p_blind_list_is_exactly_where_the_timestamps_coincide():
    for name, kind, scen in K.RUNS:
        if not K.CASES[name].rel_bias:
            continue
        b = K.batch(name, kind, scen)
        N = K.CASES[name].N
        rows = torch.arange(b.ts.shape[0])
        same = bool((b.ts[rows, b.positions] == b.ts[rows, torch.clamp(b.positions + 1, max=N - 1)]).all())
        assert same == ((name, kind, scen) in TS_P_BLIND), (name, kind, scen)


@pytest.mark.parametrize("run", K.RUNS, ids=K.run_id)
def test_bars_reject_plausible_decode_bugs(run):
    name, kind, scen = run
    d = K.direct(*run)
    for bug in R.BUGS + R.GEMV_BUGS:
        if not applicable(name, kind, scen, bug):
            continue
        bad = K.direct_mutant(name, kind, scen, bug)
        margin = {q: float((bad[q] - d.ref64[q]).abs().max()) / d.bars[q] for q in K.QUANTITIES}
        assert max(margin.values()) > 1.0, (run, bug, margin, d.bars)


def test_decode_supported_is_the_restated_lds_bound():
    from rails_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    grid = set(itertools.product((0, 1, 9), (1, 64, 1024, 1025), (1, 2, 8, 52, 53, 4096, 4097), (1, 31, 32, 33), (1, 32, 33), (0, 1, 255, 256)))
    for good, bad in K.BOUNDARY_PAIRS.values():
        assert K.supported(*good) and not K.supported(*bad), (good, bad)
        grid |= {good, bad}
    for c in K.CASES.values():
        grid.add((c.N, c.D, c.H, c.dqk, c.dv, c.buckets))
    assert K.lds_bytes(64, 52, 32, 32, 0) <= K.LDS_BYTES < K.lds_bytes(64, 53, 32, 32, 0)
    for N, D, H, dqk, dv, nb in sorted(grid):
        assert lib.rails_hstu_decode_supported(N, D, H, dqk, dv, nb) == int(K.supported(N, D, H, dqk, dv, nb)), (N, D, H, dqk, dv, nb)
