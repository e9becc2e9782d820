"""Writes tests/golden/sampler_restatements.npz: the values of restatement_values() (tests/test_keyed_perm_cpu.py) — this
project's own numpy restatements of the device samplers, the words digest and the store-file header — as they were before the
restatements moved into r2l_amd/keyed_perm.py and r2l_amd/store_file.py.  Run from the repository root; a re-run on a tree
that passes the test writes the same arrays."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests.test_keyed_perm_cpu import restatement_values  # noqa: E402

np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "sampler_restatements.npz"), **restatement_values())
