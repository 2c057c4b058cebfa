"""Writes tests/golden/conv_choices.json: what hawq_conv2d_choice, hawq_conv2d_splitk_ok and hawq_conv2d_splitk_workspace
answer for every case of tests/conv_choice_cases.py, from whatever library HAWQ_LIB names.

The committed fixture was recorded from the commit BEFORE the dispatcher was split into check / choose / launch, patched so
that hawq_conv2d returns at its launch site (profiles/conv_dispatch_refactor.md quotes the patch):

    HAWQ_LIB=/path/to/that/libhawq_mi355.so python tests/golden/make_conv_choices.py

The answers are interned and "choices" is one flat list: an accepted case is two numbers l, a >= 0 - the launch half of
hawq_conv_choice (family .. lds_bytes) is "launch"[l], the kernel-argument half (stride .. ring_bytes) is "args"[a] - and
a refused one is the single number -(t + 1) with "texts"[t] = [rc, error text].
The generator refuses to write a fixture that does not resolve every tile id, reach every function-table slot and show
every refusal text of hawq_conv2d.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from hawq_amd import _lib  # noqa: E402
from tests import conv_choice_cases as cases  # noqa: E402

OUT = os.path.join(HERE, "conv_choices.json")

# function-table slots per family: (fn_table, fn[0], fn[1], fn[2]) with -1 for unused indices
SLOTS = {
    0: {(0, e, v, -1) for e in range(4) for v in range(3)} | {(1, v, -1, -1) for v in range(5)} |
       {(2, e, v, -1) for e in range(2) for v in range(2)} | {(3, v, -1, -1) for v in range(2)},
    1: {(0, n, t, r) for n in range(2) for t in range(2) for r in range(2)},
    2: {(0, t, r, -1) for t in range(2) for r in range(2)},
    3: {(0, n, r, t) for n in range(2) for r in range(2) for t in range(2)} | {(1, n, -1, -1) for n in range(2)},
    4: {(0, n, e, t) for n in range(2) for e in range(3) for t in range(2)} | {(1, n, -1, -1) for n in range(2)},
}
# slots no valid argument struct reaches (profiles/conv_dispatch_refactor.md says why); their instantiations stay
UNREACHABLE = {}   # family -> slots; empty: the case list reaches every slot at the commit the fixture was recorded from


def record(lib, a):
    out = _lib.ConvChoice()
    rc = lib.hawq_conv2d_choice(C.byref(a), C.byref(out))
    if rc:
        return [rc, lib.hawq_last_error().decode()]
    row = []
    for n, _ in _lib.ConvChoice._fields_:
        v = getattr(out, n)
        row.extend(list(v) if n == "fn" else [v])
    return row


def record_splitk(lib, a, s):
    slab, cnt = C.c_int64(-1), C.c_int64(-1)
    ok = lib.hawq_conv2d_splitk_ok(C.byref(a), s)
    rc = lib.hawq_conv2d_splitk_workspace(C.byref(a), s, C.byref(slab), C.byref(cnt))
    return [ok, rc, slab.value, cnt.value] if rc == 0 else [ok, rc, lib.hawq_last_error().decode()]


def names_digest(names):
    return hashlib.sha256("\n".join(names).encode()).hexdigest()[:16]


N_LAUNCH = 10   # family, tile, index, fn_table, fn[3], grid, block, lds_bytes


def expand(doc):
    """The recorded choices with the interned halves and refusal texts in place: what record() returns for each case."""
    flat, out = iter(doc["choices"]), []
    for x in flat:
        out.append(doc["texts"][-x - 1] if x < 0 else doc["launch"][x] + doc["args"][next(flat)])
    return out


def collect(lib):
    all_cases = cases.build_cases()
    sk = cases.splitk_cases()
    null_args = [lib.hawq_conv2d_choice(None, C.byref(_lib.ConvChoice())), lib.hawq_last_error().decode()]
    choices = [record(lib, a) for _, a in all_cases]
    texts = sorted({tuple(r) for r in choices if len(r) == 2})
    launch = sorted({tuple(r[:N_LAUNCH]) for r in choices if len(r) > 2})
    args = sorted({tuple(r[N_LAUNCH:]) for r in choices if len(r) > 2})
    return {
        "fields": [n for n, _ in _lib.ConvChoice._fields_],
        "cases": names_digest([n for n, _ in all_cases]),
        "texts": texts, "launch": launch, "args": args,
        "choices": [x for r in choices for x in ([launch.index(tuple(r[:N_LAUNCH])), args.index(tuple(r[N_LAUNCH:]))] if len(r) > 2 else [-texts.index(tuple(r)) - 1])],
        "null_args": null_args,
        "splitk_cases": names_digest([n for n, _, _ in sk]),
        "splitk": [record_splitk(lib, a, s) for _, a, s in sk],
    }


def check_coverage(doc):
    choices = expand(doc)
    rows = [r for r in choices if len(r) > 2]
    texts = [t for _, t in doc["texts"]] + [doc["null_args"][1]]
    tiles = {r[1] for r in rows}
    assert tiles == set(range(1, cases.NUM_TILES + 1)), f"tile ids never resolved: {sorted(set(range(1, cases.NUM_TILES + 1)) - tiles)}"
    for fam, slots in SLOTS.items():
        seen = {tuple(r[3:7]) for r in rows if r[0] == fam}
        missing = slots - seen - set(UNREACHABLE.get(fam, ()))
        assert not missing, f"family {fam}: function-table slots never reached: {sorted(missing)}"
        assert seen <= slots, f"family {fam}: slots outside the tables: {sorted(seen - slots)}"
    for text in cases.REQUIRE_TEXTS:
        assert any(text in t for t in texts), f"refusal text never seen: {text!r}"
    for i, (text, _, _) in enumerate(cases.INVALID):
        got = choices[len(choices) - len(cases.INVALID) + i]
        assert len(got) == 2 and text in got[1], f"invalid case {i} should be refused with {text!r}, got {got}"


def main():
    lib = _lib.load()
    doc = collect(lib)
    doc = json.loads(json.dumps(doc))   # tuples -> lists, as a reader of the file sees them
    check_coverage(doc)
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    n_ok = sum(len(r) > 2 for r in expand(doc))
    print(f"{OUT}: {len(expand(doc))} cases ({n_ok} accepted), {len(doc['splitk'])} split-K cases, {os.path.getsize(OUT)} bytes from {_lib.library_path()}")


if __name__ == "__main__":
    main()
