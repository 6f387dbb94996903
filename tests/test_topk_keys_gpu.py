"""The exact top-k kernels of topk.hip against the 64-bit key order, bit for bit, on every route of topk() and on the shard merge.

Every case of tests/_topk_ref.py's table first asserts -- on the CPU, from the restated dispatch and thread layout -- that it still takes the
route and the branch it is there for, then runs the entry point and compares score words (as int32 views) and ids exactly with the
restatement.  Rows are bit patterns (+-0, subnormals, NaNs of both signs with payloads, +-inf); each call gets an odd leading dimension, so
rows 1 and up start off 16-byte alignment, sits inside a buffer of guard values that must come back untouched, and -- where the entry point
takes its outputs -- writes into sentinel-filled outputs.  tests/test_topk_keys_cpu.py shows that these bars can fail."""
import numpy as np
import pytest
import torch

from rails_amd import engine as E
from tests import _topk_ref as T

pytestmark = pytest.mark.gpu

GUARD = 0x7F7FFFFF          # FLT_MAX around every input row: a kernel that read a guard column would rank it near the top
SENT_SCORE = 0x7FC0DEAD     # what the outputs hold before the call
SENT_ID = -777777
FRONT = 8                   # guard values before row 0 (row 0 stays 16-byte aligned, rows 1 and up do not: the leading dimension is odd)


def dev():
    return torch.device("cuda", 0)


def _device_rows(bits):
    rows, n = bits.shape
    ld = n + 3 if (n + 3) % 2 else n + 4
    host = np.full(FRONT + rows * ld + 8, GUARD, dtype=np.uint32)
    for r in range(rows):
        host[FRONT + r * ld: FRONT + r * ld + n] = bits[r]
    buf = torch.from_numpy(host.view(np.int32)).to(dev())
    return buf, host, buf.view(torch.float32).as_strided((rows, n), (ld, 1), FRONT)


def _outputs(rows, k):
    s = torch.full((rows, k), SENT_SCORE, dtype=torch.int32, device=dev()).view(torch.float32)
    i = torch.full((rows, k), SENT_ID, dtype=torch.int64, device=dev())
    return s, i


def _words(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _assert_rows(case, got_s, got_i, want_s, want_i):
    got_s, got_i = _words(got_s), got_i.cpu().numpy()
    for r in range(want_s.shape[0]):
        ok_s, ok_i = np.array_equal(got_s[r], want_s[r]), np.array_equal(got_i[r], want_i[r])
        if not (ok_s and ok_i):
            bad = np.flatnonzero((got_s[r] != want_s[r]) | (got_i[r] != want_i[r]))
            j = int(bad[0])
            fam = case.rows[r % len(case.rows)]
            raise AssertionError(f"{case.name} row {r} {fam}: {bad.shape[0]} of {want_s.shape[1]} places differ, first at {j}: got "
                                 f"(0x{int(got_s[r, j]):08X}, {int(got_i[r, j])}), the key order gives (0x{int(want_s[r, j]):08X}, {int(want_i[r, j])})")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _flag(case):
    return None if case.run_if is None else torch.tensor([case.run_if], dtype=torch.int32, device=dev())


def _filtered(case, sel_s, sel_ids):
    inv = T.case_invalid(case, sel_ids)
    rows = sel_s.shape[0]
    want_i = np.zeros((rows, case.k_out), dtype=np.int64)
    want_s = np.zeros((rows, case.k_out), dtype=np.uint32)
    for r in range(rows):
        want_i[r], want_s[r] = T.filter_seen(sel_ids[r], sel_s[r], inv[r], case.k_out)
    return inv, want_s, want_i


def _run_selection(case, index):
    bits = T.case_rows(case)
    name, _ = T.case_route(case)
    assert name == case.route, f"{case.name} is there for {case.route}, the dispatch now sends it to {name}"
    if case.want:
        T.check_wants(case, T.case_tags(case, bits)[1])
    rows = bits.shape[0]
    sel_s, sel_pos = T.case_selection(case, bits)
    mode, table = T.case_ids(case, index)
    sel_ids = np.stack([T.map_ids(mode, table, r, sel_pos[r]) for r in range(rows)])
    buf, host, view = _device_rows(bits)
    if case.entry == "topk":
        out_s, out_i = _outputs(rows, case.k)
        E.topk(view, case.k, ids=_t(table) if mode != "positions" else None, out=(out_s, out_i), run_if=_flag(case))
        want_s, want_i = sel_s, sel_ids
    elif case.entry == "topk_filtered":
        inv, want_s, want_i = _filtered(case, sel_s, sel_ids)
        out_s, out_i = _outputs(rows, case.k_out)
        E.topk_filtered(view, case.k, _t(table) if mode != "positions" else None, _t(inv), case.k_out, out=(out_i, out_s), run_if=_flag(case))
    elif case.entry == "topk_candidates":
        positions, ids = table
        out_s, out_i = E.topk_candidates(view, case.k, _t(positions), _t(ids))
        want_s, want_i = sel_s, sel_ids
    else:
        positions, ids = table
        inv, want_s, want_i = _filtered(case, sel_s, sel_ids)
        out_i, out_s = E.topk_candidates_filtered(view, case.k, _t(positions), _t(ids), _t(inv), case.k_out)
    if case.run_if == 0:        # the launch predicate kept every kernel of the route from running
        want_s, want_i = np.full_like(want_s, SENT_SCORE), np.full_like(want_i, SENT_ID)
    _assert_rows(case, out_s, out_i, want_s, want_i)
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), host), f"{case.name}: the input rows or their guard columns were written"


def _run_merge(case):
    msg = T.case_messages(case)
    R, k, rows = case.R, case.n, msg.shape[1]
    assert T.lists_sorted(msg, R, k) == (not case.unsorted)
    gathered = _t(msg.reshape(R * rows, 2 * k))
    if case.entry == "merge":
        want_s, want_i = T.merged(msg, R, k, case.k)
        out_s, out_i = E.merge_candidates(gathered, R, k, case.k)
    else:
        sel_s, sel_i = T.merged(msg, R, k, case.k)
        inv, want_s, want_i = _filtered(case, sel_s, sel_i)
        out_i, out_s = E.merge_candidates_filtered(gathered, R, k, case.k, _t(inv), case.k_out)
    _assert_rows(case, out_s, out_i, want_s, want_i)
    assert np.array_equal(gathered.cpu().numpy(), msg.reshape(R * rows, 2 * k))


@pytest.mark.parametrize("index", range(len(T.CASES)), ids=[c.name for c in T.CASES])
def test_topk_is_the_key_order(index):
    case = T.CASES[index]
    if case.route == "merge":
        _run_merge(case)
    else:
        _run_selection(case, index)


def test_merged_shards_are_the_unsharded_selection():
    """Shard-major positions carry the tie rule over: the per-shard selections of a row with special values and ties, merged, are the
    selection of the whole row -- both computed on the device, compared with the restatement of the whole row."""
    R, shard, k = 4, 1500, 200
    case = T.Case(name="shards", entry="topk", n=R * shard, k=k, rows=(("low_byte", {}), ("nans", {}), ("signed_zeros", {})), route="row_select")
    bits = T.case_rows(case)
    msg = np.zeros((R, bits.shape[0], 2 * k), dtype=np.int64)
    for r in range(R):
        _, _, view = _device_rows(bits[:, r * shard: (r + 1) * shard])
        s, i = E.topk(view, k)
        msg[r, :, :k] = _words(s).astype(np.int64)
        msg[r, :, k:] = i.cpu().numpy() + r * shard
    out_s, out_i = E.merge_candidates(_t(msg.reshape(R * bits.shape[0], 2 * k)), R, k, k)
    want_s, want_pos = T.case_selection(case, bits)
    _assert_rows(case, out_s, out_i, want_s, want_pos)
