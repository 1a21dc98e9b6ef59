"""Live-stream micro-batching with an order-preserving re-publisher.

The reference handles one frame per subscriber callback — decode, one
blocking RPC, postprocess, publish (``communicator/ros_inference.py:117-175``;
the 3D subscriber's queue of 50 at ``communicator/ros_inference3d.py:110``
buys nothing because the callback still takes one cloud at a time).  Here the
subscriber callback only enqueues:

* :class:`LatestWinsWindow` — a bounded window of the newest messages; when
  the pipeline falls behind, the OLDEST pending frames are dropped (a live
  detector should publish the present, not a growing backlog).
* :class:`MicroBatchRunner` — ``workers`` threads each take every pending
  message up to ``batch`` in one go and run them as ONE engine call (one
  graph replay / one DP scatter over the node's GPUs per micro-batch).
  With ``workers > 1`` host work of one batch (JPEG decode, message
  building) overlaps another batch's device work.
* :class:`OrderedRepublisher` — results are released in dispatch order
  (tickets are handed out atomically with the take), and a result whose
  ``header.seq`` is not newer than the last one published is dropped, so the
  published stream's ``header.seq`` is strictly increasing whatever order
  the batches finish in.  An optional ``ordered_fn`` is the stage that must see
  the stream in order (a tracker): called once per ticket, in ticket order,
  under the re-publisher's lock, with that ticket's items that survived the
  stale-seq filter, it returns the items to publish.
"""
from __future__ import annotations

import collections
import threading
from typing import Callable, Dict, List, Optional, Sequence


def _seq_of(msg) -> Optional[int]:
    h = getattr(msg, "header", None)
    return getattr(h, "seq", None) if h is not None else None


class LatestWinsWindow:
    def __init__(self, capacity: int):
        self.capacity = max(1, int(capacity))
        self.q: collections.deque = collections.deque()
        self.cv = threading.Condition()
        self.closed = False
        self.dropped = 0

    def put(self, msg) -> None:
        with self.cv:
            if len(self.q) >= self.capacity:
                self.q.popleft()
                self.dropped += 1
            self.q.append(msg)
            self.cv.notify_all()  # the condition is shared with wait_idle()

    def take_locked(self, max_n: int) -> List:
        n = min(max_n, len(self.q))
        return [self.q.popleft() for _ in range(n)]

    def close(self) -> None:
        with self.cv:
            self.closed = True
            self.cv.notify_all()

    def __len__(self) -> int:
        with self.cv:
            return len(self.q)


class OrderedRepublisher:
    """submit(ticket, [(seq, item), ...]) → publish_fn(item) in ticket order,
    dropping items whose seq is not newer than the last published one.  With an
    ``ordered_fn`` the surviving items of a ticket go through it first (one call per
    ticket, in ticket order, under the lock) and what it returns is published; an
    exception it raises is kept in ``errors`` and that ticket publishes nothing."""

    def __init__(self, publish_fn: Callable, ordered_fn: Optional[Callable[[List], List]] = None,
                 errors: Optional[List[BaseException]] = None):
        self.publish_fn = publish_fn
        self.ordered_fn = ordered_fn
        self.errors: List[BaseException] = errors if errors is not None else []
        self.next = 0
        self.pending: Dict[int, Sequence] = {}
        self.lock = threading.Lock()
        self.last_seq: Optional[int] = None
        self.published = 0
        self.stale = 0

    def submit(self, ticket: int, items: Sequence) -> None:
        with self.lock:
            self.pending[ticket] = items
            while self.next in self.pending:
                if self.ordered_fn is not None:
                    self._release_ordered(self.pending.pop(self.next))
                    self.next += 1
                    continue
                for seq, item in self.pending.pop(self.next):
                    if seq is not None and self.last_seq is not None and seq <= self.last_seq:
                        self.stale += 1
                        continue
                    self.publish_fn(item)
                    self.published += 1
                    if seq is not None:
                        self.last_seq = seq
                self.next += 1

    def _release_ordered(self, items: Sequence) -> None:
        keep = []
        for seq, item in items:
            if seq is not None and self.last_seq is not None and seq <= self.last_seq:
                self.stale += 1
                continue
            keep.append(item)
            if seq is not None:
                self.last_seq = seq
        try:
            out = self.ordered_fn(keep)
        except BaseException as e:  # keep the stream alive, like a failed batch
            self.errors.append(e)
            return
        for item in out:
            self.publish_fn(item)
            self.published += 1


class MicroBatchRunner:
    """process_fn(list of messages) → list of (seq, publishable) in message order."""

    def __init__(self, process_fn: Callable[[List], List], publish_fn: Callable, batch: int = 8,
                 capacity: Optional[int] = None, workers: int = 1,
                 ordered_fn: Optional[Callable[[List], List]] = None):
        self.batch = max(1, int(batch))
        self.window = LatestWinsWindow(capacity or self.batch * max(1, workers) * 2)
        self.errors: List[BaseException] = []
        self.repub = OrderedRepublisher(publish_fn, ordered_fn, self.errors)
        self.process_fn = process_fn
        self._ticket = 0
        self._inflight = 0
        self.batches = 0
        self.threads = [threading.Thread(target=self._run, name=f"tca-batch-{i}", daemon=True)
                        for i in range(max(1, workers))]
        for t in self.threads:
            t.start()

    def push(self, msg) -> None:
        self.window.put(msg)

    def _run(self) -> None:
        w = self.window
        while True:
            with w.cv:
                while not w.q and not w.closed:
                    w.cv.wait()
                if not w.q and w.closed:
                    return
                msgs_ = w.take_locked(self.batch)
                msgs_.sort(key=lambda m: (_seq_of(m) is None, _seq_of(m) or 0))
                ticket = self._ticket
                self._ticket += 1
                self._inflight += 1
            try:
                out = self.process_fn(msgs_)
                items = [(_seq_of(m), o) for m, o in zip(msgs_, out)]
            except BaseException as e:  # keep the stream alive; surfaced to the caller / tests
                self.errors.append(e)
                items = []
            self.repub.submit(ticket, items)
            with w.cv:
                self.batches += 1
                self._inflight -= 1
                w.cv.notify_all()

    def wait_idle(self, timeout: float = 60.0) -> bool:
        """Block until the window is empty and no batch is in flight."""
        with self.window.cv:
            return self.window.cv.wait_for(lambda: not self.window.q and self._inflight == 0, timeout)

    def close(self, drain: bool = True, timeout: float = 60.0) -> None:
        if drain:
            self.wait_idle(timeout)
        self.window.close()
        for t in self.threads:
            t.join(timeout=timeout)
