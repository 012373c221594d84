#!/usr/bin/env python
"""
make_engine_settings.py — records tests/golden/engine_settings.json: what every combination of the engines' settings
(tests/_engine_settings_cases.py) is answered with — accepted and what the plan then carries, or the refusal's type and text —
through model.engine(**kw) and through engine.configure(**kw).  tests/test_engine_settings_cpu.py replays the file.

The file is a record of the engines AS THEY WERE when it was made: run this on the commit whose behaviour is to be kept, not
after a change to the rules (a change that is meant shows up as a failing replay, and is then recorded here on purpose).
    python tests/golden/make_engine_settings.py
No device is needed.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _engine_settings_cases as sc  # noqa: E402


def main():
    table = sc.record()
    data = sc.pack(table)
    assert sc.unpack(data) == json.loads(json.dumps(table))
    path = os.path.join(HERE, "engine_settings.json")
    with open(path, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    flat = [o for v in table["constructor"].values() for o in v]
    print("constructor: %d cases, %d accepted, %d distinct messages in all; configure: %d cases; %d bytes"
          % (len(flat), sum(o[0] == "ok" for o in flat), len(data["messages"]),
             sum(len(r) for v in table["configure"].values() for r in v), os.path.getsize(path)))


if __name__ == "__main__":
    main()
