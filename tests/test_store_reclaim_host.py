"""The history of tests/test_gpu_store_reclaim.py on the model alone: its
coverage conditions, and ReclaimModel.reclaim against keys.reclaim, the host
statement of honu_key_reclaim, at every reclaim of the history. No GPU."""
import functools

import pytest

import store_model as sm
import store_reclaim as sr
from honu_amd import keys
from honu_amd.metadata import SEEK_NONE
from honu_amd.workload import gen_host_batch


@functools.lru_cache(maxsize=None)
def gen(seed, n):
    return gen_host_batch(seed, "small", 0, n)


@pytest.fixture(scope="module")
def marshal(oracle_lib):
    return oracle_lib.marshal_batch


def reclaim_both_ways(model):
    """The model's reclaim, and keys.reclaim over the state it had."""
    order, valid = model.order(), model.valid
    values = [r[2] for r in model.records]
    col_keys = list(model.keys())
    got = keys.reclaim(order, valid, values, keys=list(model.keybytes))
    live_bytes = model.live_bytes()
    want = model.reclaim()
    order_out, remap, source, values_out, keys_out, _, _ = got
    assert source == want["source"] and [r for r in range(len(remap)) if remap[r] == SEEK_NONE] == want["freed"]
    assert order_out[:valid] == model.order() and order_out[valid:] == [SEEK_NONE] * (len(order) - valid)
    assert values_out == [r[2] for r in model.records] and keys_out == model.keybytes
    assert model.keys() == col_keys and model.tail == [] and model.valid == model.n == len(source)
    assert sum(len(v) for v in values_out) == live_bytes == model.live_bytes()
    return want


def test_history_covers_what_it_says(marshal):
    hist = sr.History()
    ma, mb = sr.ReclaimModel(marshal), sr.ReclaimModel(marshal)
    log = {}
    for model, steps in ((ma, hist.steps), (mb, hist.peer)):
        for step in steps:
            if step["kind"] == "reclaim":
                before = sm.expectations(model, hist.probes)
                log[step["name"]] = reclaim_both_ways(model)
                after = sm.expectations(model, hist.probes)
                # the column and every read give the same keys and the same record bytes
                assert before["keys"] == after["keys"] and before["hit_records"] == after["hit_records"]
                assert before["versions"] == after["versions"] and before["tops"] == after["tops"]
                assert before["obj_off"] == after["obj_off"] and after["n"] == after["valid"] == before["valid"]
            else:
                sr.apply_step(model, step, gen)
            if step["name"] in ("01 create", "02 update"):
                assert 1400 <= len(step["requests"][0]) <= 1600
    assert len(log["04 reclaim"]["batches"]) >= 2 and len(log["04 reclaim"]["freed"]) >= 900
    assert log["09 reclaim"]["equal"] >= 40
    assert log["11 reclaim"]["freed"] == []
    assert len(log["p4 reclaim"]["freed"]) >= 100
    # the ship: later versions and objects the peer lacks, padded to cap with empty records the peer then frees
    cmp = ma.compare(mb)
    assert cmp.counts[1] >= 5 and cmp.counts[2] >= 5
    mb.batch += 1
    visits, idx = ma.ship(mb, ma.n)
    assert 100 <= len(idx) < ma.n
    assert len(reclaim_both_ways(mb)["freed"]) == ma.n - len(idx)
