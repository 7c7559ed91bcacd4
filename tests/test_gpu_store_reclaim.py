"""A store that gives memory back, on the GPU against the store model.

tests/test_gpu_store_rounds.py runs a store of only device state against a
dict-and-list model; that store only grows. Here the same store with
honu_key_reclaim (tests/store_reclaim.py) runs one history in which records
are freed three times and written, deleted, compacted and shipped in between:
after every step the store's whole state and every read path are compared with
the model, as there. The coverage conditions are asserted on the model.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import store_model as sm  # noqa: E402
import store_reclaim as sr  # noqa: E402
from honu_amd.metadata import INFO_DTYPE  # noqa: E402
from test_gpu_store_rounds import (check_batch, check_compare, check_model, check_shipped, codecs, gen, h,  # noqa: E402,F401
                                   marshal)


def run(store, model, steps, probes, d_probes, marshal, log):
    """The steps on the model and on the store, everything compared after each."""
    for step in steps:
        kind = step["kind"]
        want = sr.apply_step(model, step, gen)
        d_status = store.probes(sm.expectations(model, probes)["live_status"])  # before the step is issued
        freed = None
        if kind == "write":
            req, status = step["requests"]
            got = store.write(step["op"], req, status, step["pid"], sm.REGION, sm.NOW + step["seed"],
                              gen(step["seed"], len(req)))
            check_batch(marshal, step, got, want)
        elif kind == "put_stored":
            check_batch(marshal, step, store.put_raw(want[0]), want)
        elif kind == "drop":
            store.drop(step["prefixes"])
            freed = want
        elif kind == "compact":
            store.compact()
            freed = want
        else:
            n_before = store.n
            kept, total = store.reclaim()
            assert kept == model.n == n_before - len(want["freed"])
            assert total == model.live_bytes() == store.rec_bytes == store.arena.numel()  # the arena is the live records
            assert int(store.rec_off[kept].item()) == total
            log.append((step["name"], want))
        check_model(store, model, probes, d_probes, freed, d_status)
        if kind == "reclaim":  # the records themselves, in the model's order, and the per-record arrays beside them
            off = h(store.rec_off)
            arena = h(store.arena)
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(r[2]) for r in model.records])]).tolist()
            assert arena.tobytes() == b"".join(r[2] for r in model.records)
            keys = h(store.keys).reshape(-1, 29)
            assert keys.tobytes() == b"".join(model.keybytes)  # after a reclaim every record is a live row
            assert (h(store.key_status) == 0).all() and store.info.numel() == 32 * model.n
            assert h(store.info, INFO_DTYPE)["tombstone"].astype(bool).tolist() == [r[1] for r in model.records]


def test_a_store_that_reclaims(codecs, marshal):  # noqa: F811
    hist = sr.History()
    ma, mb = sr.ReclaimModel(marshal), sr.ReclaimModel(marshal)
    a, b = sr.ReclaimStore(codecs[0]), sr.ReclaimStore(codecs[1])
    pa, pb = a.probes(hist.probes), b.probes(hist.probes)
    log = []
    run(a, ma, hist.steps, hist.probes, pa, marshal, log)
    run(b, mb, hist.peer, hist.probes, pb, marshal, [])

    # the coverage conditions
    by = dict(log)
    assert len(by["04 reclaim"]["batches"]) >= 2 and len(by["04 reclaim"]["freed"]) >= 900  # two batches' records go
    assert by["09 reclaim"]["equal"] >= 40                       # freed records whose keys are byte-equal to live ones
    assert by["11 reclaim"]["freed"] == [] and ma.tail == []     # and a reclaim with nothing to free
    assert all(len(w["freed"]) > 0 for name, w in log[:2])

    # the first ships to the second, which has itself reclaimed: record indices on both sides are the new ones
    cap = a.n
    want_cmp = ma.compare(mb)
    mb.batch += 1
    visits, idx = ma.ship(mb, cap)
    got = a.ship_to(b)
    torch.cuda.synchronize()
    c = check_compare(got.compared, want_cmp)
    assert c["later"] >= 5 and c["only_mine"] >= 5
    sent = check_shipped(ma, got, visits, idx)
    assert sent >= 100
    status = h(b.key_status)[got.first:got.first + cap]
    assert (status[:sent] == 0).all() and (status[sent:] != 0).all()  # the empty records past the total
    check_model(b, mb, hist.probes, pb)
    # and the second frees the empty records the ship appended
    want = mb.reclaim()
    kept, total = b.reclaim()
    assert len(want["freed"]) == cap - sent and kept == mb.n and total == mb.live_bytes()
    check_model(b, mb, hist.probes, pb)
