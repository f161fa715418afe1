"""The prefix cache's salt (``Scheduler.add(..., salt=)``): sequences with different salts never
share pages even for equal tokens -- the serving engine salts a request with its LoRA adapter slot,
because the cached K/V depend on the adapter that computed them.  Salt 0 is the default and is what
tests/test_prefix_cache.py covers."""

import numpy as np
import pytest

from dstack_amd.serving._native import Scheduler

PAGE = 64


def _sched(mask=None):
    s = Scheduler(num_pages=32, page_size=PAGE, max_batch=8, max_prefill_tokens=4096, max_model_len=1024,
                  enable_prefix_caching=True)
    if mask is not None:
        s._test_set_hash_mask(mask)  # 0: every page hash collides, the stored ids and salt decide
    return s


def _ids(n, seed):
    return np.random.default_rng(seed).integers(1, 1000, size=n).astype(np.int32)


def _prefill(s, sid, ids, **kw):
    s.add(sid, len(ids), len(ids) + 50, ids, **kw)
    p = s.schedule()
    assert p["kind"] == "prefill" and list(p["seq_ids"]) == [sid]
    s.mark_computed(sid)
    s.append(sid, 7)
    return p


@pytest.mark.parametrize("mask", [None, 0])
def test_salt_separates_equal_tokens(mask):
    a = _ids(200, 0)
    s = _sched(mask)
    assert list(_prefill(s, 1, a, salt=1)["starts"]) == [0]
    assert s.cached_pages == 3
    # other salts (0 among them): no hit, and their own pages are registered next to the first ones
    assert list(_prefill(s, 2, a, salt=2)["starts"]) == [0]
    assert list(_prefill(s, 3, a)["starts"]) == [0]
    assert s.cached_pages == 9 and s.prefix_hit_tokens == 0
    assert not set(s.pages(1)[:3]) & set(s.pages(2)[:3]) and not set(s.pages(2)[:3]) & set(s.pages(3)[:3])
    # the same salt hits its own pages, whichever sequences are still running
    for sid, salt, owner in ((4, 1, 1), (5, 2, 2), (6, 0, 3)):
        p = _prefill(s, sid, a, salt=salt)
        assert list(p["starts"]) == [192] and list(p["lens"]) == [8]
        assert list(p["block_tables"][0][:3]) == s.pages(owner)[:3]
    assert s.prefix_hit_tokens == 3 * 192 and s.cached_pages == 9


@pytest.mark.parametrize("mask", [None, 0])
def test_salt_survives_release_and_preemption_style_readmission(mask):
    a = _ids(130, 1)
    s = _sched(mask)
    _prefill(s, 1, a, salt=5)
    s.finish(1)  # its two full pages stay cached under salt 5
    assert s.cached_pages == 2
    assert list(_prefill(s, 2, a, salt=6)["starts"]) == [0]
    s.finish(2)
    assert list(_prefill(s, 3, a, salt=5)["starts"]) == [128]
    assert list(_prefill(s, 4, a, salt=6)["starts"]) == [128]
    # a longer prompt continues the salted chain: its third page registers under the same salt
    b = np.concatenate([a, _ids(100, 2)])
    assert list(_prefill(s, 5, b, salt=5)["starts"]) == [128]
    assert list(_prefill(s, 6, b, salt=5)["starts"]) == [192]
    assert list(_prefill(s, 7, b, salt=6)["starts"]) == [128]


def test_salt_zero_is_the_default():
    a = _ids(200, 3)
    s = _sched()
    _prefill(s, 1, a)
    assert list(_prefill(s, 2, a, salt=0)["starts"]) == [192]
    t = _sched()
    _prefill(t, 1, a, salt=0)
    assert list(_prefill(t, 2, a)["starts"]) == [192]
    assert s.pages(1)[:3] == t.pages(1)[:3] and s.cached_pages == t.cached_pages == 3
