"""dspfun_amd -- MI355X-native real-even DCT engine for the dspfun tools' hot path.

Only what the path needs: csrc/ (HIP kernels + the C ABI of include/dspfft.h and include/fftw3.h)
and thin host-side mirrors of the reference call sites.
"""
from .engine import Plan, DspfftError, REDFT01, REDFT10, set_plan_effort, ScanFrames, scan_frame_rgb, trc_apply, trc_id, motion_grid_plans, motion_temporal_plans, motion_spec_constants, motion_spec_blocks, motion_ispec_blocks, spec_image_plans, spec_image_params  # noqa: F401
