"""tests/slab_ranks.py without a GPU: the ranks' "device memory" is one numpy byte array per rank, addresses are offsets
into it (past BASE, so that none is 0), and the copy functions are numpy copies.  The callbacks are called through their
ctypes function pointers, as the device library calls them."""
import threading
import time

import numpy as np
import pytest

from slab_ranks import COMM_SLOTS, RankGroup

BASE = 4096


def fake_device(P, nbytes, rng):
    mem = [rng.integers(0, 256, nbytes, dtype=np.uint8) for _ in range(P)]

    def copy_out(r, host, addr):
        host[:] = mem[r][addr - BASE:addr - BASE + host.size]

    def copy_in(r, addr, host):
        mem[r][addr - BASE:addr - BASE + host.size] = host

    return mem, copy_out, copy_in


@pytest.mark.parametrize("P", [1, 2, 3, 4, 8])
def test_three_forms_deliver_the_all_to_all(P):
    """forms 1, 2 and 3 (whole chunks, then strided pieces with bytes < stride at an offset, then a second piece at
    another base: the side array) move exactly the bytes the header names and no others"""
    rng = np.random.default_rng(P)
    chunk, side = 96, 8                      # bytes per peer of the rows and of the side array
    send0, recv0 = BASE, BASE + P * chunk + 64
    side_send, side_recv = recv0 + P * chunk + 64, recv0 + P * chunk + 64 + P * side + 32
    total = side_recv + P * side + 32 - BASE
    mem, copy_out, copy_in = fake_device(P, total, rng)
    group = RankGroup(P, copy_out, copy_in, timeout=20.0)
    calls = [(1, send0, recv0, chunk, 0, chunk, -1),          # whole array
             (2, send0, recv0, chunk, 0, chunk, 5),
             (3, send0, recv0, chunk, 24, 40, 7),             # a piece: bytes < stride, at an offset
             (3, side_send, side_recv, side, 2, 4, 7 + COMM_SLOTS)]  # the side array's piece of the same exchange
    for form, send, recv, stride, offset, n, slot in calls:
        for m in mem:
            m[:] = rng.integers(0, 256, m.size, dtype=np.uint8)
        before = [m.copy() for m in mem]
        want = [m.copy() for m in mem]
        for r in range(P):
            for q in range(P):
                src = send - BASE + q * stride + offset
                dst = recv - BASE + r * stride + offset
                want[q][dst:dst + n] = before[r][src:src + n]

        def rank(r):
            cb = group.callbacks(r)
            if form == 1:
                return cb.exchange(None, send, recv, n)
            if form == 2:
                return cb.start(None, send, recv, n, slot) or cb.wait(None, slot)
            return cb.piece(None, send, recv, stride, offset, n, slot) or cb.wait(None, slot)

        assert group.run(rank) == [0] * P
        for r in range(P):
            assert np.array_equal(mem[r], want[r]), (form, r)
            assert group.starts(r)[-1] == (form, slot, stride, offset, n)
        assert any(not np.array_equal(b, m) for b, m in zip(before, mem))  # (random bytes: something moved)
    assert group.log[0] == [(1, -1, chunk, 0, chunk), (2, 5, chunk, 0, chunk), ("wait", 5, 0, 0, 0), (3, 7, chunk, 24, 40),
                            ("wait", 7, 0, 0, 0), (3, 7 + COMM_SLOTS, side, 2, 4), ("wait", 7 + COMM_SLOTS, 0, 0, 0)]


def test_slot_books():
    """a wait for a slot that is not in flight, and a start on one that is, fail the exchange"""
    mem, copy_out, copy_in = fake_device(1, 256, np.random.default_rng(0))
    group = RankGroup(1, copy_out, copy_in)
    cb = group.callbacks(0)
    assert cb.start(None, BASE, BASE + 128, 16, 3) == 0
    assert cb.start(None, BASE, BASE + 128, 16, 3) == 1
    assert isinstance(group.error, AssertionError) and "started again" in str(group.error)
    group = RankGroup(1, copy_out, copy_in)
    assert group.callbacks(0).wait(None, 3 + COMM_SLOTS) == 1
    assert isinstance(group.error, AssertionError) and "not in flight" in str(group.error)


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_numpy_model_of_the_slab_transform(P):
    """per rank: rfft along x and fft along y of the local planes, packed [peer][nz local][nyl][nx/2] with the x-Nyquist
    column apart as [peer][nz local][nyl] (the side array), the group's all-to-all of both pieces, fft along the global z:
    together np.fft.rfftn of the global array.  ny / P = 3 is odd."""
    nx, nyl, nzl = 10, 3, 2
    ny, nz, nxm = nyl * P, nzl * P, nx // 2
    rng = np.random.default_rng(11 + P)
    a = rng.standard_normal((nz, ny, nx))
    rows, side = nzl * nyl * nxm * 16, nzl * nyl * 16       # bytes per peer
    send0, recv0, side_send, side_recv = (BASE + i * P * rows for i in range(4))
    mem, copy_out, copy_in = fake_device(P, 4 * P * rows, rng)
    group = RankGroup(P, copy_out, copy_in, timeout=20.0)

    def rank(r):
        cb = group.callbacks(r)
        s = np.fft.fft(np.fft.rfft(a[r * nzl:(r + 1) * nzl], axis=2), axis=1)          # [nz local][ny][nx/2 + 1]
        packed = s.reshape(nzl, P, nyl, nxm + 1).transpose(1, 0, 2, 3)                  # [peer][nz local][nyl][..]
        mem[r][send0 - BASE:send0 - BASE + P * rows] = np.ascontiguousarray(packed[..., :nxm]).view(np.uint8).reshape(-1)
        mem[r][side_send - BASE:side_send - BASE + P * side] = np.ascontiguousarray(packed[..., nxm]).view(np.uint8).reshape(-1)
        assert cb.piece(None, send0, recv0, rows, 0, rows, 0) == 0
        assert cb.piece(None, side_send, side_recv, side, 0, side, COMM_SLOTS) == 0
        t = np.empty((nz, nyl, nxm + 1), np.complex128)                                 # [sender][nz local] = [nz global]
        t[..., :nxm] = mem[r][recv0 - BASE:recv0 - BASE + P * rows].view(np.complex128).reshape(nz, nyl, nxm)
        t[..., nxm] = mem[r][side_recv - BASE:side_recv - BASE + P * side].view(np.complex128).reshape(nz, nyl)
        return np.fft.fft(t, axis=0)

    got = np.concatenate(group.run(rank), axis=1)
    ref = np.fft.rfftn(a)
    assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_a_rank_that_raises_frees_the_others(form):
    """rank 1 raises before its first exchange: every other rank's callback returns non-zero well within the time-out, no
    thread stays alive, and run() re-raises that rank's exception"""
    P = 4
    mem, copy_out, copy_in = fake_device(P, 1024, np.random.default_rng(0))
    group = RankGroup(P, copy_out, copy_in, timeout=20.0)
    returned = [None] * P

    def rank(r):
        if r == 1:
            raise ValueError("rank 1 fails")
        cb = group.callbacks(r)
        returned[r] = (cb.exchange(None, BASE, BASE + 512, 16) if form == 1 else
                       cb.start(None, BASE, BASE + 512, 16, 0) if form == 2 else
                       cb.piece(None, BASE, BASE + 512, 16, 0, 16, 0))

    before = threading.active_count()
    t0 = time.monotonic()
    with pytest.raises(ValueError, match="rank 1 fails"):
        group.run(rank)
    assert time.monotonic() - t0 < 10.0
    assert returned == [1, None, 1, 1]
    assert group.alive == 0 and threading.active_count() == before
    assert group.callbacks(0).exchange(None, BASE, BASE + 512, 16) == 1  # and the group stays failed
