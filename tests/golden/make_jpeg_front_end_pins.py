"""Writes tests/golden/jpeg_front_end_parser.json and tests/golden/jpeg_front_end_planner.json: what ``hawq_amd.jpeg`` does today with
mutated fixture files (``parse_jpeg``, with and without ``progressive=True``) and which bytes its two planners write, as computed by
tests/jpeg_pins.py.  tests/test_jpeg_front_end_pins.py holds a later ``hawq_amd/jpeg.py`` to them.

    python tests/golden/make_jpeg_front_end_pins.py

Run it on the revision whose behaviour is to be kept, never to make a failing test pass.  It needs jpeg_cases.npz, jpeg_sync_cases.npz
and jpeg_prog_cases.npz (make_jpeg_cases.py, make_jpeg_sync_cases.py, make_jpeg_prog_cases.py) and no GPU.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from tests import jpeg_pins

    parser, planner = jpeg_pins.parser_pins(), jpeg_pins.planner_pins()
    assert parser["inputs"] >= 15000 and parser["reasons"] >= 25 and 5 * parser["accepted"] >= parser["inputs"], {k: parser[k] for k in ("inputs", "reasons", "accepted")}
    for name, pins in (("jpeg_front_end_parser.json", parser), ("jpeg_front_end_planner.json", planner)):
        path = os.path.join(HERE, name)
        with open(path, "w") as f:
            json.dump(pins, f, indent=0, sort_keys=True)
            f.write("\n")
        print(path, os.path.getsize(path), "bytes")
    print({k: parser[k] for k in ("inputs", "reasons", "accepted")}, len(planner), "plans")


if __name__ == "__main__":
    main()
