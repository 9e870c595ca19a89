"""Background writer of the predicted volumes (--save_predict): the evaluator hands over a case's volume -- already in
NIfTI file order, on the device or on the host -- and goes on with the next case while ONE thread of this process writes the
352-byte header and the gzip stream (zlib releases the interpreter lock while it deflates).

Device volumes come back in one copy each: into one of two pinned host buffers (grown to the largest case seen), on a
side stream that waits for an event recorded on the producer's stream after the compose.  At most two cases are pending
(queued or being written) at any time -- one per buffer; `submit` blocks beyond that.  An exception raised in the thread is
kept and re-raised in the caller by the next `submit` or by `close()`; the cases queued behind the failed one are dropped.
"""
import queue
import threading

import numpy as np

from ..data import nii_kits

MAX_PENDING = 2


class VolumeWriter(object):
    def __init__(self):
        self._slots = threading.Semaphore(MAX_PENDING)
        self._queue = queue.Queue()
        self._error = None
        self._thread = None
        self._closed = False
        self._lock = threading.Lock()
        self._pinned = [None] * MAX_PENDING
        self._stream = None
        self._count = 0
        self.pending = 0                # submitted and not yet written
        self.max_pending = 0
        self.written = []               # paths, in the order they were finished

    # ------------------------------------------------------------------ caller side
    def _raise_pending_error(self):
        if self._error is not None:
            err, self._error = self._error, None
            raise err

    def _reserve(self, block):
        """One of the two places; what the thread met so far is raised here."""
        if self._closed:
            raise RuntimeError("the volume writer is closed")
        self._raise_pending_error()
        if not self._slots.acquire(blocking=block):
            raise queue.Full("{} volumes are pending".format(MAX_PENDING))
        if self._error is not None:                         # met while this call waited
            self._slots.release()
            self._raise_pending_error()

    def _put(self, path, fn):
        with self._lock:
            self.pending += 1
            self.max_pending = max(self.max_pending, self.pending)
        if self._thread is None:
            self._thread = threading.Thread(target=self._work, name="volume-writer", daemon=True)
            self._thread.start()
        self._queue.put((str(path), fn))

    def submit(self, path, header, shape, flat, block=True):
        """Write `flat` (file order, prod(shape) elements) to `path` with `header`'s geometry.  flat: a numpy array (kept by
        reference: the caller must not change it) or a dense 1-D device tensor, which is copied into this place's pinned
        buffer on a side stream that waits for what the caller's stream holds now; the caller's stream does not wait.
        block=False raises queue.Full instead of waiting for one of the two places."""
        if isinstance(flat, np.ndarray):
            self._reserve(block)
            self._put(path, lambda: nii_kits.save_flat(flat, shape, header, path))
            return
        import torch
        if not flat.is_cuda or not flat.is_contiguous() or flat.dim() != 1:
            raise ValueError("a dense 1-D device tensor expected, got {} on {}".format(tuple(flat.shape), flat.device))
        self._reserve(block)                # places are served in order: the case that used this buffer last is written
        try:
            slot, n = self._count % MAX_PENDING, flat.numel()
            buf = self._pinned[slot]
            if buf is None or buf.numel() < n or buf.dtype != flat.dtype:
                buf = self._pinned[slot] = torch.empty(n, dtype=flat.dtype, pin_memory=True)
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=flat.device)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(flat.device))
            done = torch.cuda.Event()
            with torch.cuda.stream(self._stream):
                self._stream.wait_event(ready)
                buf[:n].copy_(flat, non_blocking=True)
                done.record(self._stream)
            flat.record_stream(self._stream)                # its memory is not handed out again before the copy ran
            host = buf[:n].numpy()
        except BaseException:
            self._slots.release()
            raise

        def job():
            done.synchronize()
            nii_kits.save_flat(host, shape, header, path)

        self._count += 1
        self._put(path, job)

    def submit_call(self, path, fn, block=True):
        """Run fn() -- which writes `path` -- in the writer thread, in order with the volumes."""
        self._reserve(block)
        self._put(path, fn)

    def join(self):
        """Wait until everything submitted so far is written (measurements: a run that does not overlap)."""
        self._queue.join()
        self._raise_pending_error()

    def close(self):
        """Finish the queue, stop the thread and re-raise what it met."""
        if not self._closed:
            self._closed = True
            if self._thread is not None:
                self._queue.put(None)
                self._thread.join()
        self._raise_pending_error()

    # ------------------------------------------------------------------ writer thread
    def _work(self):
        while True:
            job = self._queue.get()
            if job is None:
                self._queue.task_done()
                return
            path, fn = job
            try:
                if self._error is None:         # behind a failed case: dropped until the caller has seen the error
                    fn()
                    self.written.append(path)
            except BaseException as err:        # kept for the caller; the thread lives on to drain the queue
                self._error = err
            finally:
                with self._lock:
                    self.pending -= 1
                self._slots.release()
                self._queue.task_done()
