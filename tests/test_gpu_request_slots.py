"""GPU test of the request slots across entry points: one ctx, 2 x
RL_REQUESTS_INFLIGHT + 1 batches with no rl_synchronize in between, alternating
between rl_do_limit_requests_packed_async, rl_do_limit_wire_async and
rl_do_limit_wire_respond_async, their request counts stepping through 0, 1, 3,
257, 2, 300: every slot is reused, and its mbuf, wbuf and cbuf grow while older
batches are in flight. A twin ctx answers the same batches through the
synchronous rl_do_limit_requests_verdict."""
import numpy as np
import pytest

from ratelimit_amd import abi
from ratelimit_amd.limiter import Backend
import test_gpu_respond as R
from test_gpu_requests import gen_requests
from test_gpu_requests_packed import INFLIGHT, assert_same, guards_intact, sync_reference, table_state
from test_gpu_wire import OK, Pair, encode, reference

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 3, 257, 2, 300]
KINDS = ["packed", "wire", "respond"]


def test_gpu_request_slots_are_reused_and_grow_across_entry_points():
    pr = Pair()  # (be: the pipelined ctx; ref_be: its twin, one hash seed)
    try:
        flight = []
        n_batches = 2 * INFLIGHT + 1
        for b in range(n_batches):
            nq, kind = COUNTS[b % len(COUNTS)], KINDS[b % len(KINDS)]
            reqs, nows = gen_requests(700 + b, nq, p_override=0.0)
            msgs = encode(reqs)
            st, a = reference(pr.pk, msgs, nows)
            assert (st == OK).all()
            n = len(a["req_idx"])
            mode = "both" if b % 2 == 0 or kind == "respond" else "out"  # verdict on for some batches, off for others
            gs = b % 4 == 1
            keys = R.STD_KEYS if b % 2 else None
            if kind == "packed":
                item = pr.fl.submit(pr.be, a, pr.n_rules, mode, gs)
            elif kind == "wire":
                item = pr.fl.submit_wire(pr.be, msgs, nows, pr.n_rules, n, mode, gs)
            else:
                item = R.submit_respond(pr.fl, pr.be, msgs, nows, pr.n_rules, n, keys, mode, gs)
            ref = sync_reference(pr.ref_be, a, pr.n_rules, "both", gs)
            flight.append((kind, mode, keys, item, ref, a, nq, n))
        # slots: batch b took slot b % INFLIGHT; what each slot saw, in order
        per_slot = [[(f[0], f[6]) for f in flight[j::INFLIGHT]] for j in range(INFLIGHT)]
        assert all(len(s) >= 2 for s in per_slot)                              # every slot reused
        assert any(x[1] < y[1] for s in per_slot for x, y in zip(s, s[1:]))    # ... by a larger batch (mbuf, cbuf)
        assert any(x[0] != "packed" and y[0] != "packed" and x[1] + 255 < y[1]
                   for s in per_slot for x, y in zip(s, s[1:]))                # ... and a wire batch's wbuf grows
        sub, done = pr.be.batch_progress()
        assert sub == n_batches
        pr.be.synchronize()
        for kind, mode, keys, item, ref, a, nq, n in flight:
            assert_same(item, ref, mode)
            if kind != "packed":
                first = np.searchsorted(a["req_idx"], np.arange(nq + 1)).astype(np.uint32)
                assert item["wire"]["req_status"][:nq].tobytes() == bytes(nq)
                assert item["wire"]["desc_first"][:nq + 1].tobytes() == first.tobytes()
                assert int(item["wire"]["n_descriptors"][0]) == n
            if kind == "respond":
                res = {k: ref[k] for k in abi.REQUEST_RESULT_DTYPES}
                ver = {k: ref[k] for k in abi.REQUEST_VERDICT_DTYPES}
                raw, off = Backend.response_serialize(first, np.zeros(nq, np.uint8), res, ver, keys)
                assert R.responses(item) == R.split(raw, off)
            guards_intact(item)
        assert pr.be.batch_progress() == (n_batches, n_batches)
        assert table_state(pr.ref_be) == table_state(pr.be)
        assert pr.be.table_info()["decisions"] > 0
    finally:
        pr.close()
