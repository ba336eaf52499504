"""The reference's answers on record, so that tests/test_oracle_vs_ref.py runs wherever the repository does.

A test asks the reference through `Recorder(case).reference(name)` instead of `Reference(name)`.  Every question -- the
constructor, a property, a method or a `lib.<function>` call, with a hash of its arguments -- and every answer go into one
sequence per test case, stored as tests/golden/vs_ref/<case>.npz (data only: the questions, the answers' dtypes and shapes,
their bytes).
  * oracle/_ref built (the reference compiled by oracle/Makefile): the reference answers, and each answer must equal the
    recorded one bit for bit -- the record is checked against the reference itself;
  * oracle/_ref absent: the record answers, after checking that each question is the one recorded at that point (same call,
    same arguments), so a test that changed its inputs fails instead of reading answers to other questions;
  * QPSK_RECORD_REF=1 with oracle/_ref built: the reference answers and the record is (re)written.
"""
import hashlib
import json
import os

import numpy as np

from oracle.pyoracle import Reference, ref_available

RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vs_ref")


def _digest(args, kwargs):
    h = hashlib.sha256()
    for a in list(args) + [kwargs[k] for k in sorted(kwargs)]:
        a = np.asarray(a)
        h.update(("%s%s" % (a.dtype, a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def _leaf(v):
    """-> (layout entry, bytes) of an array or scalar answer"""
    if isinstance(v, np.generic):
        a = np.asarray(v)
        return ["s", str(a.dtype), []], a.tobytes()
    if isinstance(v, (bool, int, float)):          # a Python number comes back as one
        a = np.asarray(v)
        return ["p", str(a.dtype), []], a.tobytes()
    a = np.ascontiguousarray(v)
    return ["a", str(a.dtype), list(a.shape)], a.tobytes()


def _encode(v):
    if v is None:
        return {"k": "n"}, b""
    if isinstance(v, dict):
        items, blob = [], b""
        for key in sorted(v):
            lay, b = _leaf(v[key])
            items.append([key] + lay)
            blob += b
        return {"k": "d", "items": items}, blob
    lay, b = _leaf(v)
    return {"k": "v", "leaf": lay}, b


def _decode_leaf(lay, blob, off):
    kind, dt, shape = lay
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
    a = np.frombuffer(blob[off:off + n], dtype=dt).reshape(shape).copy()
    return {"s": lambda: a[()], "p": lambda: a.item(), "a": lambda: a}[kind](), off + n


def _decode(layout, blob):
    if layout["k"] == "n":
        return None
    if layout["k"] == "d":
        out, off = {}, 0
        for item in layout["items"]:
            out[item[0]], off = _decode_leaf(item[1:], blob, off)
        return out
    return _decode_leaf(layout["leaf"], blob, 0)[0]


class Recorder:
    def __init__(self, case):
        self.path = os.path.join(RECORDS, case + ".npz")
        self.live = ref_available("c1small")
        self.recording = self.live and os.environ.get("QPSK_RECORD_REF") == "1"
        self.pos = 0
        self.questions, self.layouts, self.blobs = [], [], []
        if not self.recording:
            assert os.path.exists(self.path), "no record %s: run with QPSK_RECORD_REF=1 where oracle/_ref is built" % self.path
            z = np.load(self.path)
            self.questions = [str(q) for q in z["questions"]]
            self.layouts = [json.loads(str(s)) for s in z["layouts"]]
            offs = np.concatenate([[0], np.cumsum(z["sizes"])])
            blob = z["blob"].tobytes()
            self.blobs = [blob[offs[i]:offs[i + 1]] for i in range(len(self.questions))]

    def ask(self, question, live_answer):
        """live_answer: a callable giving the reference's own answer (called only where the reference is here)"""
        if self.recording:
            v = live_answer()
            lay, b = _encode(v)
            self.questions.append(question)
            self.layouts.append(lay)
            self.blobs.append(b)
            return v
        i = self.pos
        assert i < len(self.questions), "question %d (%s) is beyond the record %s" % (i, question, self.path)
        assert self.questions[i] == question, "question %d: asked %s, recorded %s" % (i, question, self.questions[i])
        self.pos += 1
        if self.live:
            v = live_answer()
            lay, b = _encode(v)
            assert lay == self.layouts[i] and b == self.blobs[i], "question %d (%s): the reference's answer differs from the record" % (i, question)
            return v
        return _decode(self.layouts[i], self.blobs[i])

    def reference(self, name):
        self.ask("Reference(%s)" % name, lambda: None)
        return _RefProxy(self, Reference(name) if self.live else None)

    def finish(self):
        if self.recording:
            os.makedirs(RECORDS, exist_ok=True)
            np.savez_compressed(self.path, questions=np.array(self.questions), layouts=np.array([json.dumps(s) for s in self.layouts]),
                                sizes=np.array([len(b) for b in self.blobs], np.int64),
                                blob=np.frombuffer(b"".join(self.blobs), np.uint8))
        else:
            assert self.pos == len(self.questions), "%d of %d recorded questions asked (%s)" % (self.pos, len(self.questions), self.path)


class _LibProxy:
    def __init__(self, rec, lib):
        self._rec, self._lib = rec, lib

    def __getattr__(self, name):
        def call(*args):
            return self._rec.ask("lib.%s(%s)" % (name, _digest(args, {})), lambda: getattr(self._lib, name)(*args))
        return call


class _RefProxy:
    """stands for one Reference(name): methods and properties of the Reference class, its constants, and `lib`"""

    def __init__(self, rec, ref):
        self._rec, self._ref = rec, ref
        self.lib = _LibProxy(rec, ref.lib if ref is not None else None)

    def __getattr__(self, name):
        if callable(getattr(Reference, name, None)):
            def call(*args, **kwargs):
                return self._rec.ask("%s(%s)" % (name, _digest(args, kwargs)), lambda: getattr(self._ref, name)(*args, **kwargs))
            return call
        return self._rec.ask(name, lambda: getattr(self._ref, name))
