"""Z-slab ranks as threads of the test process (a plain module, imported by name from tests/ like gpu_buffers.py).

RankGroup(P, copy_out, copy_in) is the all-to-all of include/kwave_hip.h between P ranks that all live in this process:
for every peer q, `bytes` at send + q * stride + offset of the sender arrive at recv + sender * stride + offset of rank q.
Every rank copies its P pieces into host memory (copy_out), the ranks meet at a threading.Barrier, every rank copies
the pieces meant for it out of the others' host memory (copy_in), and they meet again before anybody's staging memory is
reused.  copy_out(rank, host uint8 array, address) and copy_in(rank, address, host uint8 array) are the ranks' own
kw_memcpy_d2h / kw_memcpy_h2d on a GPU (device_copies) and plain numpy copies in the CPU tests: no kernel of one rank
ever waits for another rank, and nothing but the barrier connects them.

callbacks(rank) holds the three callback forms of the header as ctypes function pointers, all on that one all-to-all:
  form 1  exchange(user, send, recv, bytes_per_peer)                              blocking, whole array
  form 2  start(user, send, recv, bytes_per_peer, slot) / wait(user, slot)       start does the copy, wait keeps the books
  form 3  piece(user, send, recv, stride, offset, bytes, slot) / wait(user, slot)
Per rank, log[rank] lists (form, slot, stride, offset, bytes) of every exchange (slot -1 for form 1) and ("wait", slot,
0, 0, 0) of every wait.  A wait of a slot that is not in flight, or a start on a slot that is, fails the exchange.

Nothing can hang: every Barrier.wait has a time-out; a rank whose function or callback raises aborts the barrier, so every
other rank's callback returns non-zero at once (the library then returns KW_ERR_COMM to that rank); run() joins the
threads with a time-out and re-raises the first exception.  P = 1 needs no threads: the same callbacks copy send to recv.
"""
import ctypes as C
import threading

import numpy as np

TIMEOUT = 60.0
COMM_SLOTS = 32  # KW_COMM_SLOTS of csrc/kw_internal.h: the side array of an exchange on `slot` travels on slot + COMM_SLOTS

CB_EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
CB_START = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)
CB_WAIT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)
CB_PIECE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int)


class RankCallbacks:
    """the callback forms of one rank; the ctypes objects live as long as this does"""

    def __init__(self, group, rank):
        g, r = group, rank
        self.exchange = CB_EXCHANGE(g._guard(lambda user, send, recv, n: g._exchange(r, 1, -1, send, recv, n, 0, n)))
        self.start = CB_START(g._guard(lambda user, send, recv, n, slot: g._exchange(r, 2, slot, send, recv, n, 0, n)))
        self.piece = CB_PIECE(g._guard(lambda user, send, recv, stride, offset, n, slot:
                                       g._exchange(r, 3, slot, send, recv, stride, offset, n)))
        self.wait = CB_WAIT(g._guard(lambda user, slot: g._wait(r, slot)))

    @staticmethod
    def address(cb):
        return C.cast(cb, C.c_void_p)


class RankGroup:
    def __init__(self, nranks, copy_out, copy_in, timeout=TIMEOUT):
        self.P, self.copy_out, self.copy_in, self.timeout = nranks, copy_out, copy_in, timeout
        self.barrier = threading.Barrier(nranks) if nranks > 1 else None
        self.stage = [np.zeros(0, np.uint8) for _ in range(nranks)]
        self.log = [[] for _ in range(nranks)]
        self.in_flight = [set() for _ in range(nranks)]
        self.error = None
        self.alive = 0  # rank threads that outlived the last run()'s join
        self._lock = threading.Lock()
        self._cbs = [RankCallbacks(self, r) for r in range(nranks)]

    def callbacks(self, rank):
        return self._cbs[rank]

    # ---- errors ---------------------------------------------------------------------------------------------------------
    def _keep(self, e):
        """the first exception wins; a broken barrier is only ever the echo of one"""
        with self._lock:
            if self.error is None or (isinstance(self.error, threading.BrokenBarrierError) and
                                      not isinstance(e, threading.BrokenBarrierError)):
                self.error = e
        if self.barrier is not None:
            self.barrier.abort()

    def _guard(self, fn):
        def call(*args):
            try:
                if self.error is not None:
                    raise threading.BrokenBarrierError()
                fn(*args)
                return 0
            except BaseException as e:  # noqa: BLE001 - must not unwind through the C frames
                self._keep(e)
                return 1
        return call

    def _meet(self):
        if self.barrier is not None:
            self.barrier.wait(self.timeout)

    # ---- the exchange ---------------------------------------------------------------------------------------------------
    def _exchange(self, r, form, slot, send, recv, stride, offset, n):
        self.log[r].append((form, slot, stride, offset, n))
        if form != 1:
            if slot in self.in_flight[r]:
                raise AssertionError(f"rank {r}: slot {slot} started again before it was waited for")
            self.in_flight[r].add(slot)
        P = self.P
        if self.stage[r].size < P * n:
            self.stage[r] = np.zeros(P * n, np.uint8)
        mine = self.stage[r]
        for q in range(P):
            self.copy_out(r, mine[q * n:(q + 1) * n], send + q * stride + offset)
        self._meet()
        for q in range(P):
            self.copy_in(r, recv + q * stride + offset, self.stage[q][r * n:(r + 1) * n])
        self._meet()

    def _wait(self, r, slot):
        self.log[r].append(("wait", slot, 0, 0, 0))
        if slot not in self.in_flight[r]:
            raise AssertionError(f"rank {r}: wait for slot {slot}, which is not in flight")
        self.in_flight[r].remove(slot)

    def forget_in_flight(self):
        """after the pipeline was destroyed: exchanges it started ahead for a consumer that never came are gone with it"""
        for s in self.in_flight:
            s.clear()

    def starts(self, rank=0, since=0):
        return [e for e in self.log[rank][since:] if e[0] != "wait"]

    # ---- the ranks ------------------------------------------------------------------------------------------------------
    def run(self, fn):
        """fn(rank) on every rank at once; returns the list of results, re-raises the first exception"""
        results = [None] * self.P
        if self.P == 1:
            try:
                results[0] = fn(0)
            except BaseException as e:  # noqa: BLE001
                self._keep(e)
        else:
            def main(r):
                try:
                    results[r] = fn(r)
                except BaseException as e:  # noqa: BLE001
                    self._keep(e)
            threads = [threading.Thread(target=main, args=(r,), daemon=True) for r in range(self.P)]
            for t in threads:
                t.start()
            for t in threads:
                t.join(self.timeout + 30.0)
            self.alive = sum(t.is_alive() for t in threads)
        if self.error is not None:
            raise self.error
        if self.alive:
            raise RuntimeError(f"{self.alive} rank threads did not finish")
        return results


def device_copies(devs):
    """(copy_out, copy_in) over the contexts devs[rank] (kwave_amd.capi.Device): the rank's own blocking copies, which are
    ordered after everything enqueued on its stream"""
    from kwave_amd import capi

    def copy_out(r, host, addr):
        capi.check(devs[r].L.kw_memcpy_d2h(devs[r].ctx, host.ctypes.data, addr, host.nbytes))

    def copy_in(r, addr, host):
        capi.check(devs[r].L.kw_memcpy_h2d(devs[r].ctx, addr, host.ctypes.data, host.nbytes))

    return copy_out, copy_in


def install(group, devs, form, nz_global):
    """put every context into slab mode with callback form 1, 2 or 3 (before kw_fused_create)"""
    adr = RankCallbacks.address
    for r, d in enumerate(devs):
        cb = group.callbacks(r)
        d.call("fused_set_slab", group.P, r, nz_global, adr(cb.exchange), None)
        if form == 2:
            d.call("fused_set_slab_async", adr(cb.start), adr(cb.wait))
        elif form == 3:
            d.call("fused_set_slab_pieces", adr(cb.piece), adr(cb.wait))
        else:
            assert form == 1, form
