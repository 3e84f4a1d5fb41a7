"""Writes tests/golden/aa_frames.npz: the oracle-made resolved 32 x 24 frames of the golden scene
(c1_scene.npz, reference camera, scale 12, default lighting) for the four store x algorithm pairs at
S = 2 and 4 samples per axis -- recorded results that tests/test_aa_ref.py holds tests/aa_ref.py to.
Run from the repository root: python -m tests.golden.make_aa_frames"""
from __future__ import annotations

import os

import numpy as np

import oracle
from tests import aa_ref

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, SCALE = 32, 24, 12
STORES = {"vcs": oracle.STORE_VCS, "hashtable": oracle.STORE_HASHTABLE}
ALGOS = {"longestaxis": oracle.ALGO_LONGESTAXIS, "original": oracle.ALGO_ORIGINAL}


def key(store: str, algo: str, S: int) -> str:
    return f"{store}_{algo}_s{S}"


def main() -> None:
    d = np.load(os.path.join(HERE, "c1_scene.npz"))
    cam, lit = oracle.reference_camera(W, H), oracle.lighting()
    frames = {}
    for sname, store in STORES.items():
        sc = oracle.Scene(d["xyz"], d["rgb"], store)
        for aname, algo in ALGOS.items():
            for S in (2, 4):
                frames[key(sname, aname, S)] = aa_ref.aa_frame(sc, algo, cam, lit, W, H, S, SCALE).reshape(H, W)
        sc.close()
    np.savez_compressed(os.path.join(HERE, "aa_frames.npz"), **frames)


if __name__ == "__main__":
    main()
