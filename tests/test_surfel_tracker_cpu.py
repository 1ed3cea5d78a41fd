"""CPU: the frame-to-model tracker (SurfelPoseEstimator) builds from a checkpoint path with PoseEstimator's overrides, from_config
dispatches on frame2frame, and the forms that cannot work frame to model (chunked, pipelined, sharded) are refused with a reason."""
import pytest
import torch
import yaml

from test_checkpoint_paths import INFER_F2F_YAML, H, W, _checkpoint


def _slam(f2f):
    slam = yaml.safe_load(INFER_F2F_YAML)['slam']
    slam['frame2frame'] = f2f
    return slam


def test_surfel_estimator_from_checkpoint_path(tmp_path):
    from rpe_amd import pose_estimator, synth
    path, cfg, sd = _checkpoint(tmp_path)
    K = synth.intrinsics(H, W)
    est = pose_estimator.SurfelPoseEstimator(_slam(False), K, 1800.0, path, (W, H))
    m = est.model
    assert tuple(m.config['image_shape']) == (H, W) and m.config['lbgfs_iters'] == 20 and m.config['use_weights'] is True
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    assert float(est.scale) == pytest.approx(1 / 250) and est.scene is None
    with pytest.raises(ValueError):
        pose_estimator.SurfelPoseEstimator(_slam(True), K, 1800.0, path, (W, H))


def test_from_config_dispatch_and_refusals(tmp_path):
    from rpe_amd import pose_estimator, sharding, synth
    path, _, _ = _checkpoint(tmp_path)
    K = synth.intrinsics(H, W)
    f2f = pose_estimator.from_config(_slam(True), K, 1800.0, path, (W, H))
    f2m = pose_estimator.from_config(_slam(False), K, 1800.0, path, (W, H))
    assert type(f2f) is pose_estimator.PoseEstimator and type(f2m) is pose_estimator.SurfelPoseEstimator
    img = torch.zeros(2, 3, H, W)
    with pytest.raises(RuntimeError, match='chunked'):
        f2m.forward_chunk(img, img, torch.ones(2, 1, H, W, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='pipelined'):
        f2m.submit(img[:1], img[:1], torch.ones(1, 1, H, W, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match='SurfelPoseEstimator'):
        pose_estimator.PoseEstimator(_slam(False), K, 1800.0, path, (W, H))
    tr = sharding.SequenceTracker(lambda: f2m, lambda t: None)
    with pytest.raises(ValueError, match='sharded'):
        tr.track(4, rank=0, world=2)
