"""Records tests/golden/receding_<case>.npz from the REFERENCE build (oracle/_ref, built by `make -C oracle ref` where the
reference sources exist): data only — per case three trajectories' solved plan, the shifted inputs, the initial roll-out
after the shift (x, clamped u, cost) and the warm solve's final cost, iteration count and return value
(tests/receding_cases.py: chain).

    python tests/golden/make_receding_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle.harness import lib_path  # noqa: E402
from receding_cases import CASES, case, chain  # noqa: E402

if __name__ == "__main__":
    for name in CASES:
        c = case(name)
        lib = lib_path("ref", c["problem"], c["fd"])
        if not os.path.exists(lib):
            sys.exit("%s is missing: the fixtures are recorded from the reference build" % lib)
        out = chain(lib, c)
        path = os.path.join(HERE, "receding_%s.npz" % name)
        np.savez_compressed(path, s=np.array(c["s"]), **out)
        print("%s: %d bytes; iterations cold %s warm %s, return values %s / %s" % (
            os.path.basename(path), os.path.getsize(path), out["plan_iters"].astype(int).tolist(),
            out["warm_iters"].astype(int).tolist(), out["plan_rc"].tolist(), out["warm_rc"].tolist()))
