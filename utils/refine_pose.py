#!/usr/bin/env python
"""Refine camera poses against a trained R2L student (localisation against a light field):

  python utils/refine_pose.py --config configs/lego_noview.txt --pretrained_ckpt <student.tar> \
      --r2l_pose_iters 200 --r2l_pose_rays 4096 --r2l_pose_noise 2,0.05 --r2l_pose_out refined.npy

Implementation: r2l_amd/refine_pose.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from r2l_amd.refine_pose import main  # noqa: E402

if __name__ == "__main__":
    main()
