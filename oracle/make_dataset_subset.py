"""Build ``tests/golden/tpims_dataset_subset.tar.xz``: the raw TPIMS files that ``tpims_fixture.npz`` was made from.

TEST INFRASTRUCTURE, run once by hand:   python oracle/make_dataset_subset.py --root <the reference's dataset/ directory>

Data files only, byte for byte, in the reference's directory layout (no code):

* ``data/tpims_location.csv``          -> the site index space;
* ``tpims_link_0322.tar.xz``           -> the 5 regional link tables;
* ``nodes/0322/node_data_*.csv``       -> the first ``N_STEPS`` timesteps (name order = time order), as make_fixtures.py reads them.

``tests/test_etl_cpu.py`` unpacks it and checks that ``regtgcn_amd.etl`` rebuilds the committed fixture from it.
"""
from __future__ import annotations

import argparse
import os
import tarfile

from make_fixtures import N_STEPS

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "tpims_dataset_subset.tar.xz")


def members(root):
    node_dir = os.path.join("nodes", "0322")
    nodes = sorted(fn for fn in os.listdir(os.path.join(root, node_dir)) if fn.startswith("node_data_") and fn.endswith(".csv"))
    return [os.path.join("data", "tpims_location.csv"), "tpims_link_0322.tar.xz"] + [os.path.join(node_dir, fn) for fn in nodes[:N_STEPS]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", required=True, help="the reference's dataset/ directory")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()

    def normalise(ti):                      # reproducible archive: no owner, no timestamps
        ti.uid = ti.gid = 0
        ti.uname = ti.gname = ""
        ti.mtime = 0
        ti.mode = 0o644
        return ti

    names = members(a.root)
    with tarfile.open(a.out, "w:xz", format=tarfile.PAX_FORMAT) as tf:
        for name in names:
            tf.add(os.path.join(a.root, name), arcname=name, recursive=False, filter=normalise)
    print(f"{len(names)} files -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
