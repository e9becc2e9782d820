#!/usr/bin/env python
"""Train the NeRF teacher (step 1 of the pipeline; the reference's `main.py --model_name nerf` training run):

  python utils/train_nerf.py --config configs/lego.txt --experiment_name NeRF__blender_lego

Implementation: r2l_amd/train_nerf.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from r2l_amd.train_nerf import main  # noqa: E402

if __name__ == "__main__":
    main()
