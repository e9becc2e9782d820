"""Drop-in module path of the reference's LLFF data layer; implementation in r2l_amd/data.py."""
from r2l_amd.data import (get_rand_pose_llff, load_llff_data, poses_avg, recenter_poses, render_path_spiral)  # noqa: F401
