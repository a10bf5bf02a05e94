#!/usr/bin/env python3
"""Record the reference's codec-frame writer on seeded inputs (TEST INFRASTRUCTURE).

Run in the build container only (the reference does not exist on the GPU box):

    python tests/golden/make_golden_voice.py     # writes tests/golden/g6_voice.npz

The reference's capture loop builds the speech codec's 690-word input from a traffic frame's symbols
with ``_extract_voice_slot_from_symbols`` (ui/modern.py:2309-2423).  The module itself needs PyQt6 and
cannot be imported, so this script reads modern.py, takes that one function out of the syntax tree,
compiles it and calls it (it reads nothing of ``self``).  Nothing is imported from PyQt6, and only
inputs and outputs are stored: per case the dibit stream, the ``position`` given (-1: none) and the
690 int16 words returned, or that None came back.

Cases: a dozen seeded dibit streams of 300..600 symbols with a position at which the slot's 255
symbols lie inside the stream (the first at 0, one ending on the stream's last symbol); a frame
without a position; a slot past the stream's end.
"""
import ast
import logging
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TETRA_REFERENCE", "/root/reference")
NAME = "_extract_voice_slot_from_symbols"

import numpy as np  # noqa: E402


def reference_writer():
    """The reference's function, compiled from its source at run time."""
    path = os.path.join(REF, "tetraear", "ui", "modern.py")
    tree = ast.parse(open(path, encoding="utf-8").read(), path)
    fn = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == NAME]
    assert len(fn) == 1, f"{NAME} not found once in {path}"
    env = {"logger": logging.getLogger("voice")}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), env)
    return env[NAME]


def cases():
    """(dibit stream uint8, position or None)."""
    out = []
    for k in range(12):
        rng = np.random.default_rng(6600 + k)
        n = int(rng.integers(300, 601))
        sym = rng.integers(0, 4, n).astype(np.uint8)
        last = 3 * (n - 255)   # the largest position whose slot ends on the stream's last symbol
        pos = 0 if k == 0 else last if k == 1 else last + 2 if k == 2 else int(rng.integers(0, last + 1))
        out.append((sym, pos))
    rng = np.random.default_rng(6650)
    out.append((rng.integers(0, 4, 400).astype(np.uint8), None))          # no position
    out.append((rng.integers(0, 4, 400).astype(np.uint8), 3 * 146))       # 146 + 255 > 400
    out.append((rng.integers(0, 4, 254).astype(np.uint8), 0))             # shorter than a slot
    return out


def main():
    fn = reference_writer()
    arrays, pos, none, words = {}, [], [], []
    for i, (sym, p) in enumerate(cases()):
        frame = {} if p is None else {"position": p}
        got = fn(None, frame, sym, 10)
        arrays[f"sym_{i}"] = sym
        pos.append(-1 if p is None else p)
        none.append(got is None)
        w = np.zeros(690, np.int16) if got is None else np.frombuffer(got, "<i2").astype(np.int16)
        assert len(w) == 690
        words.append(w)
        print(f"case {i:2d}: {len(sym)} symbols, position {p}, " + ("None" if got is None else f"{len(got)} bytes"))
    np.savez_compressed(os.path.join(HERE, "g6_voice.npz"), **arrays, position=np.array(pos, np.int64),
                        none=np.array(none), words=np.stack(words), numpy_version=np.array(np.__version__))


if __name__ == "__main__":
    main()
