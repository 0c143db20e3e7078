"""flow_supervisor_amd: the RAFT hot path of iwbn/flow-supervisor rebuilt for MI355X (gfx950).

Layout mirrors the reference's PyTorch tree so it drops in:
    flow_supervisor_amd.core.corr      CorrBlock, AlternateCorrBlock     (pytorch/core/corr.py)
    flow_supervisor_amd.core.update    BasicUpdateBlock, SmallUpdateBlock (pytorch/core/update.py)
    flow_supervisor_amd.core.raft      RAFT (+ upsample_flow)             (pytorch/core/raft.py)
    flow_supervisor_amd.core.utils.utils  coords_grid, bilinear_sampler, upflow8, InputPadder
    flow_supervisor_amd.alt_cuda_corr  forward / backward                 (pytorch/alt_cuda_corr)
    flow_supervisor_amd.evaluate       validate_chairs / _sintel / _kitti / _kitti2012, create_*_submission, FlowMetrics
                                                                          (pytorch/evaluate.py)
    flow_supervisor_amd.unsup_loss     UnsupervisedLoss, census_loss, smoothness_loss, range_map, occlusion_mask
                                                                          (raft/unsup_loss.py, raft/smurf_models/smurf_utils.py)
    flow_supervisor_amd.selfsup_loss   SmurfLoss, self_supervision_loss, brox_occlusion_mask, fb_consistency_mask
                                                                          (the same two files: selfsup and 'brox')
    flow_supervisor_amd.augment        UnsupAugmentor, apply, as_step_input, add_noise
                                                                          (pytorch/raft_utils/augmentor.py:496-657)
                                       FlowAugmentor, SparseFlowAugmentor, apply_supervised      (augmentor.py:39-330)
The compute lives in csrc/*.hip behind the C ABI of include/fsraft.h (libfsraft.so).
"""
