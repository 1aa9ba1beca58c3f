"""Recorded answers of the reference (oracle/_ref), so that the tests pinned to it run everywhere.

A test asks its tape for every value it takes from the reference, in a fixed order:
  * ``tape.scalars(fn)`` -- a tuple of scalars (a Delta S, an acceptance flag, ...);
  * ``tape.array(fn, shape)`` -- a small array (a starting worldline, an RNG state);
  * ``tape.digest(fn)`` -- a 64-bit digest of an array (a worldline after a move, a table, a run of random numbers).
Where oracle/_ref is built (``tape.ref`` is the live reference), ``fn`` runs it and its answer is also compared with
the tape in tests/golden/ref_tapes/ (a stale tape fails); PIGS_RECORD_REF_TAPES=1 writes the tape instead.  Elsewhere
``tape.ref`` is None, ``fn`` is not called and the recorded answer is returned, so every comparison the test makes is
still made, against what the reference answered when the tape was recorded."""
import hashlib
import os
import re

import numpy as np

TAPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tapes")
RECORD = os.environ.get("PIGS_RECORD_REF_TAPES") == "1"


def canon(a):
    """float64 copy in which equal values have equal bits (same_bits semantics: -0.0 == 0.0, every NaN alike)."""
    a = np.array(a, dtype=np.float64, copy=True).ravel() + 0.0
    a[np.isnan(a)] = np.nan
    return a


def digest(a):
    """64-bit digest of canon(a) as two exactly representable float64 halves."""
    h = hashlib.sha256(canon(a).tobytes()).digest()
    return (float(int.from_bytes(h[:4], "little")), float(int.from_bytes(h[4:8], "little")))


def rng_array(mti, mt):
    """An MT19937 state (position, 624 words) as one float64 array (every value exact)."""
    return np.concatenate([[float(mti)], np.asarray(mt, np.uint32).astype(np.float64)])


def _same(a, b):
    a, b = canon(a), canon(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class RefTape:
    def __init__(self, nodeid, ref=None):
        mod, _, name = nodeid.rpartition("::")
        mod = os.path.splitext(os.path.basename(mod))[0]
        self.path = os.path.join(TAPES, "%s.%s.npz" % (mod, re.sub(r"[^A-Za-z0-9_.-]", "_", name)))
        self.ref = ref
        self.live = ref is not None
        self.recorded = []
        self.pos = 0
        self.stored = None
        if not (self.live and RECORD):
            assert os.path.exists(self.path), "no recorded reference answers: %s (record them with oracle/_ref built " \
                                              "and PIGS_RECORD_REF_TAPES=1)" % self.path
            d = np.load(self.path)
            ends = np.cumsum(d["lens"])
            self.stored = np.split(d["vals"], ends[:-1]) if len(ends) else []

    def _next(self, got):
        if self.stored is None:
            self.recorded.append(canon(got))
            return got
        assert self.pos < len(self.stored), "the test asks the reference more often than the tape recorded (%s)" % self.path
        want = self.stored[self.pos]
        self.pos += 1
        if got is not None:
            assert _same(got, want), "the reference no longer answers what %s recorded (answer %d)" % (self.path, self.pos - 1)
        return want

    def scalars(self, fn):
        """fn() -> scalar or tuple of scalars; returned as a tuple of Python floats."""
        got = np.array(np.atleast_1d(fn()), np.float64) if self.live else None
        return tuple(float(x) for x in self._next(got))

    def array(self, fn, shape):
        """fn() -> array of `shape`; live: that array itself (the reference may go on changing it in place)."""
        if self.live:
            a = fn()
            self._next(np.asarray(a, np.float64))
            return a
        return self._next(None).reshape(shape)

    def digest(self, fn):
        got = np.array(digest(fn())) if self.live else None
        return tuple(self._next(got))

    def finish(self):
        if self.stored is None:
            os.makedirs(TAPES, exist_ok=True)
            lens = np.array([len(r) for r in self.recorded], np.int32)
            vals = np.concatenate(self.recorded) if self.recorded else np.zeros(0)
            np.savez_compressed(self.path, vals=vals, lens=lens)
        else:
            assert self.pos == len(self.stored), "the test asked the reference %d times, the tape holds %d (%s)" % (
                self.pos, len(self.stored), self.path)
