"""``StatusLedger`` (monogs_amd/raster_status.py) driven with CPU int32 tensors: the host bookkeeping of the rasteriser's status
words needs no device.  One case per rule the ledger keeps."""
import pytest
import torch

from monogs_amd.raster_status import (HINTS_MAX, PENDING_MAX, STATUS_CAPACITY_OVERFLOW, STATUS_DEPTH_SORT_TIMEOUT,
                                      STATUS_TILE_SORT_TIMEOUT, StatusLedger)

A, B, C = (1024, 64, 64), (1025, 64, 64), (7, 64, 64)


def word(v=0):
    return torch.tensor([v], dtype=torch.int32)


def test_eager_overflow_doubles_the_hint_of_its_key_only():
    L = StatusLedger()
    L.remember_hint(A, 3000)
    L.remember_hint(B, 300)
    L.remember_hint(C, 5)
    L.record_capacity(A, word(STATUS_CAPACITY_OVERFLOW), capturing=False)
    L.record_capacity(B, word(STATUS_CAPACITY_OVERFLOW), capturing=False)
    L.record_capacity(C, word(0), capturing=False)
    assert L.check() is True
    assert L.hint(A) == 6000 and L.hint(B) == 1024 and L.hint(C) == 5         # max(2 * hint, 1024)
    assert L.pending == []
    assert L.check() is False
    # a key without a hint (its entry fell out of the bounded table) restarts at 1024
    L.forget_hint(A)
    L.record_capacity(A, word(STATUS_CAPACITY_OVERFLOW), capturing=False)
    assert L.check() is True and L.hint(A) == 1024


@pytest.mark.parametrize("bits,names", [(STATUS_DEPTH_SORT_TIMEOUT, ["depth sort"]), (STATUS_TILE_SORT_TIMEOUT, ["tile sort"]),
                                        (STATUS_DEPTH_SORT_TIMEOUT | STATUS_TILE_SORT_TIMEOUT, ["depth sort", "tile sort"])])
def test_sort_timeouts_raise_naming_the_sort_and_clear_the_state(bits, names):
    L = StatusLedger()
    L.remember_hint(A, 3000)
    L.record_capacity(A, word(bits), capturing=False)
    L.record_exact(B, word(0), 0, 11)
    with pytest.raises(RuntimeError) as e:
        L.check()
    for n in ("depth sort", "tile sort"):
        assert (n in str(e.value)) == (n in names)
    assert L.pending == [] and L.exact_pending is None and L.exact_other == [] and L.exact_failed == 0
    assert L.check() is False
    assert L.hint(A) == 3000
    # the same bit in an exact word
    L.record_exact(B, word(bits), 0, 11)
    with pytest.raises(RuntimeError, match=names[0]):
        L.check()
    assert L.check() is False


def test_two_handles_own_their_words():
    L = StatusLedger()
    L.remember_hint(A, 3000)
    L.remember_hint(B, 3000)
    a, b = L.graph_flags(), L.graph_flags()
    wa, wb = word(0), word(0)
    with a:
        L.record_capacity(A, wa, capturing=True)
    with b:
        L.record_capacity(B, wb, capturing=True)
    assert len(a) == 1 and len(b) == 1 and L.pending == []
    assert L.check() is False
    wb.fill_(STATUS_CAPACITY_OVERFLOW)
    assert L.check() is True                                  # with overflow in B ...
    assert L.hint(A) == 3000 and L.hint(B) == 6000            # ... only B's key is doubled
    assert L.check() is True and L.hint(B) == 12000           # a captured word stays: a replay rewrites it, every check reads it
    wb.fill_(0)
    a.release()
    wa.fill_(STATUS_CAPACITY_OVERFLOW)
    assert L.check() is False and L.hint(A) == 3000           # A's word is no longer read
    assert L.captured_words() == [(B, wb)]
    b.release()
    assert L.captured_words() == []
    a.release()
    b.release()                                               # twice is harmless
    assert L.captured_words() == [] and L.check() is False
    with pytest.raises(RuntimeError, match="released"):
        with a:
            pass


def test_nested_handles_route_to_the_innermost():
    L = StatusLedger()
    a, b = L.graph_flags(), L.graph_flags()
    with a:
        L.record_capacity(A, word(), capturing=True)
        with b:
            L.record_capacity(B, word(), capturing=True)
        L.record_capacity(A, word(), capturing=True)
        L.record_capacity(C, word(), capturing=False)         # not capturing: an eager word, whatever handle is open
    assert [k for k, _ in a.words] == [A, A] and [k for k, _ in b.words] == [B] and [k for k, _ in L.pending] == [C]


def test_accumulate_replaces_the_handles_own_last_entry():
    L = StatusLedger()
    L.remember_hint(A, 3000)
    L.remember_hint(B, 3000)
    a, b = L.graph_flags(), L.graph_flags()
    with pytest.raises(RuntimeError, match="no forward"):
        a.accumulate(word(0))
    wb = word(0)
    with b:
        L.record_capacity(B, wb, capturing=True)
    with pytest.raises(RuntimeError, match="no forward"):     # a still has none: b's entry is not a's to rewrite
        a.accumulate(word(0))
    assert b.words == [(B, wb)]
    first, own, sticky = word(0), word(STATUS_CAPACITY_OVERFLOW), word(0)
    with a:
        L.record_capacity(A, first, capturing=True)
        L.record_capacity(A, own, capturing=True)
        a.accumulate(sticky)                                  # sticky |= word, as an op of the capture
    assert int(sticky.item()) == STATUS_CAPACITY_OVERFLOW
    assert len(a) == 2 and a.words[0][1] is first and a.words[1] == (A, sticky) and b.words == [(B, wb)]
    sticky.zero_()
    own.fill_(STATUS_TILE_SORT_TIMEOUT)                       # the old word's tensor is no longer read
    assert L.check() is False
    sticky.fill_(STATUS_CAPACITY_OVERFLOW)
    assert L.check() is True and L.hint(A) == 6000 and L.hint(B) == 3000


def test_capture_without_a_handle_goes_to_the_anonymous_handle():
    L = StatusLedger()
    L.remember_hint(A, 3000)
    named = L.graph_flags()
    w1, w2 = word(0), word(0)
    L.record_capacity(A, w1, capturing=True)
    with named:
        L.record_capacity(B, w2, capturing=True)
    L.record_capacity(A, word(0), capturing=True)
    assert len(named) == 1 and len(L.captured_words()) == 3 and L.pending == []
    w1.fill_(STATUS_CAPACITY_OVERFLOW)
    assert L.check() is True and L.hint(A) == 6000
    L.release_all()                                           # what clear_graph_flags() calls
    assert L.captured_words() == [] and named.released and len(named) == 0
    assert L.check() is False
    L.record_capacity(A, w1, capturing=True)                  # a fresh anonymous handle afterwards
    assert L.captured_words() == [(A, w1)] and L.check() is True


def test_exact_word_rides_only_on_its_own_device_and_stream():
    L = StatusLedger()
    w0, w1, w2 = word(0), word(0), word(0)
    assert L.exact_rider(0, 11) is None
    L.exact_rider_read(0)
    L.record_exact(A, w0, 0, 11)
    assert L.exact_rider(0, 11) is w0 and L.exact_other == []         # same (device, stream): offered
    assert L.exact_pending is not None                               # ... and kept until the read-back happened
    L.exact_rider_read(0)
    assert L.exact_pending is None
    L.record_exact(A, w1, 0, 11)
    assert L.exact_rider(0, 12) is None                              # another stream: parked
    assert L.exact_pending is None and [e[1] for e in L.exact_other] == [w1]
    L.exact_rider_read(0)
    L.record_exact(A, w2, 0, 12)
    assert L.exact_rider(1, 12) is None                              # another device: parked
    assert [e[1] for e in L.exact_other] == [w1, w2]
    # a timeout found at the read-back is raised there and the word is forgotten
    L.record_exact(A, word(0), 1, 12)
    assert L.exact_rider(1, 12) is not None
    with pytest.raises(RuntimeError, match="tile sort"):
        L.exact_rider_read(STATUS_TILE_SORT_TIMEOUT)
    assert L.exact_pending is None
    w1.fill_(STATUS_DEPTH_SORT_TIMEOUT)                               # parked words are read by the check
    with pytest.raises(RuntimeError, match="depth sort"):
        L.check()
    assert L.exact_other == [] and L.check() is False


def test_parked_words_are_read_not_dropped_and_raised_once_by_the_next_forward():
    L = StatusLedger()
    words = [word(0) for _ in range(PENDING_MAX + 1)]
    words[3].fill_(STATUS_TILE_SORT_TIMEOUT)                          # in the oldest half
    words[PENDING_MAX - 1].fill_(STATUS_DEPTH_SORT_TIMEOUT)           # in the half that stays parked
    for i, w in enumerate(words):                                    # every forward on a stream of its own
        assert L.exact_rider(0, i) is None
        L.exact_rider_read(0)
        if i < PENDING_MAX:
            assert L.exact_failed == 0 and len(L.exact_other) == i
        L.record_exact(A, w, 0, i)
    assert len(L.exact_other) == PENDING_MAX
    assert L.exact_rider(0, -1) is None                               # parks one more than the bound: the oldest half is READ
    assert len(L.exact_other) == PENDING_MAX + 1 - PENDING_MAX // 2
    assert L.exact_other[0][1] is words[PENDING_MAX // 2]
    assert L.exact_failed == STATUS_TILE_SORT_TIMEOUT                 # its timeout bit survives
    with pytest.raises(RuntimeError, match="tile sort") as e:         # the next forward outside a capture raises it ...
        L.raise_failures()
    assert "depth sort" not in str(e.value)
    L.raise_failures()                                                # ... once
    assert L.exact_failed == 0
    with pytest.raises(RuntimeError, match="depth sort"):             # the words still parked wait for the check
        L.check()
    assert L.check() is False


def test_collected_failures_are_also_raised_by_the_check():
    L = StatusLedger()
    L.exact_failed = STATUS_DEPTH_SORT_TIMEOUT
    with pytest.raises(RuntimeError, match="depth sort"):
        L.check()
    assert L.check() is False
    L.raise_failures()


def test_eager_list_drops_its_oldest_half_unread_beyond_the_bound():
    """Today's policy, pinned: words nobody checks are dropped, not read (the parked exact words above are read)."""
    L = StatusLedger()
    L.remember_hint(A, 3000)
    for i in range(PENDING_MAX + 1):                                  # overflow and a timeout in every word of the oldest half
        bad = STATUS_CAPACITY_OVERFLOW | STATUS_TILE_SORT_TIMEOUT if i < PENDING_MAX // 2 else 0
        assert len(L.pending) == i
        L.record_capacity(A, word(bad), capturing=False)
    assert len(L.pending) == PENDING_MAX + 1 - PENDING_MAX // 2
    assert L.exact_failed == 0
    assert L.check() is False and L.hint(A) == 3000                   # nothing of the dropped half was seen
    L.raise_failures()


def test_hints_are_bounded_oldest_first():
    L = StatusLedger()
    for i in range(HINTS_MAX):
        L.remember_hint((i, 64, 64), 100 + i)
    assert len(L.hints) == HINTS_MAX
    L.remember_hint((0, 64, 64), 7)                                   # a known key is updated in place: nothing leaves
    assert len(L.hints) == HINTS_MAX and L.hint((0, 64, 64)) == 7 and L.hint((1, 64, 64)) == 101
    L.remember_hint((HINTS_MAX, 64, 64), 1)
    assert len(L.hints) == HINTS_MAX and L.hint((0, 64, 64)) is None and L.hint((1, 64, 64)) == 101
    L.remember_hint((HINTS_MAX + 1, 64, 64), 1)
    assert L.hint((1, 64, 64)) is None and L.hint((2, 64, 64)) == 102 and L.hint((HINTS_MAX, 64, 64)) == 1
