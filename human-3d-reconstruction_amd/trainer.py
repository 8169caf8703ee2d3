"""The training side of the reference's HMRTrainer (trains/trainer.py:140-323) for what trains here: the output heads on the frozen
backbone (heads.TrainableHeads), the fused losses (losses.loss_multi_pose / loss_obj_detection) and the one-launch Adam step
(optim.Adam).  NetworkTrainer (below) is the same loop over the whole network under autograd (train_model.TrainableDLASeg, BatchNorm
folded).  Printing, `debug`, the logger and the data loaders are the caller's."""
import time

import torch

from . import checkpoint, losses, optim
from .heads import TrainableHeads
from .train_model import TrainableDLASeg


def _opt(opt, name, default):
    return getattr(opt, name, default)


class ModelWithLoss(torch.nn.Module):
    """HMRModelWithLoss (trainer.py:140-149)."""

    def __init__(self, model, loss):
        super().__init__()
        self.model = model
        self.loss = loss

    def forward(self, batch):
        outputs = self.model(batch["input"])
        loss, loss_stats = self.loss(outputs, batch)
        return outputs[-1], loss, loss_stats


class AverageMeter:
    """utils/utils.py: the running average weighted by n."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        if self.count > 0:
            self.avg = self.sum / self.count


class HeadsTrainer:
    """opt: task ('multi_pose' | 'ctdet'), lr (opts.py:78, 1.25e-4), lr_step (opts.py:79, [90, 120]), num_iters (opts.py:83, -1 = the
    whole loader), device, and what the task's loss reads.  model: a model.dla_net(...) in 'f32' or 'f16x3' on the device.
    smpl_model (smpl.SMPLModel) and kp_regressor (smpl_loss.KeypointRegressor), both given and opt.smpl_kp_weight > 0 (multi_pose only):
    the loss is smpl_loss.loss_multi_pose_smpl, which adds the keypoint reprojection loss on the SMPL output and so trains the `pose`,
    `shape` and `cam` (3 channels) heads the model must then have; otherwise nothing changes.
    smpl_model given and any of opt.smpl_pose_weight / smpl_shape_weight / smpl_j3d_weight > 0 (multi_pose only): the loss is
    smpl_sup.loss_multi_pose_smpl3d -- the rotation, shape and 3D-joint terms against the batch's six SMPL label tensors
    (smpl_sup.smpl_targets), the keypoint term as well when it is switched on as above; the model must have `pose` and `shape` (and `cam`
    with the keypoint term)."""

    MODULE = TrainableHeads         # what trains: the module type behind `self.heads`

    def __init__(self, opt, model, smpl_model=None, kp_regressor=None):
        self.opt = opt
        self.model = model
        self.smpl_model = smpl_model
        self.heads = self._build_module(model)
        task = _opt(opt, "task", "multi_pose")
        kp_on = kp_regressor is not None and _opt(opt, "smpl_kp_weight", 0) > 0
        if task == "multi_pose" and smpl_model is not None and any(_opt(opt, w, 0) > 0 for w in ("smpl_pose_weight", "smpl_shape_weight", "smpl_j3d_weight")):
            from . import smpl_sup
            want = dict({"pose": 72, "shape": 10}, **({"cam": 3} if kp_on else {}))
            if any(model.heads.get(h) != c for h, c in want.items()):
                raise ValueError("HeadsTrainer: the SMPL 3D supervision needs the heads %s, the model has %s" % (want, dict(model.heads)))
            self.loss = smpl_sup.loss_multi_pose_smpl3d(opt, smpl_model, kp_regressor if kp_on else None)
        elif task == "multi_pose" and smpl_model is not None and kp_on:
            from . import smpl_loss
            want = {"pose": 72, "shape": 10, "cam": 3}
            if any(model.heads.get(h) != c for h, c in want.items()):
                raise ValueError("HeadsTrainer: the keypoint reprojection loss needs the heads %s, the model has %s" % (want, dict(model.heads)))
            self.loss = smpl_loss.loss_multi_pose_smpl(opt, smpl_model, kp_regressor)
        elif task == "multi_pose":
            self.loss = losses.loss_multi_pose(opt)
        elif task == "ctdet":
            self.loss = losses.loss_obj_detection(opt)
        else:
            raise ValueError("HeadsTrainer: task %r not defined" % (task,))
        self.loss_stats = list(self.loss.KEYS)
        self.model_with_loss = ModelWithLoss(self.heads, self.loss)
        self.lr = _opt(opt, "lr", 1.25e-4)
        self.lr_step = list(_opt(opt, "lr_step", [90, 120]))
        self.optimizer = optim.Adam(self.heads.parameters(), self.lr)

    def _build_module(self, model):
        return self.MODULE(model)

    def train_step(self, batch):
        """forward, loss.mean(), zero_grad(), backward(), step() (trainer.py:262-267) -> (output, loss, loss_stats)."""
        output, loss, loss_stats = self.model_with_loss(batch)
        loss = loss.mean()
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return output, loss, loss_stats

    def run_epoch(self, phase, epoch, data_loader):
        """trainer.py:231-301 without the printing: -> ({loss key: average weighted by batch size, 'time': minutes}, results)."""
        train = phase == "train"
        self.model_with_loss.train(train)
        opt = self.opt
        results = {}
        avg_loss_stats = {k: AverageMeter() for k in self.loss_stats}
        num_iters = _opt(opt, "num_iters", -1)
        if num_iters < 0:
            num_iters = len(data_loader)
        device = _opt(opt, "device", None)
        start = time.time()
        for iter_id, batch in enumerate(data_loader):
            if iter_id >= num_iters:
                break
            if device is not None:
                batch = {k: (v.to(device=device, non_blocking=True) if k != "meta" and torch.is_tensor(v) else v) for k, v in batch.items()}
            if train:
                output, loss, loss_stats = self.train_step(batch)
            else:
                with torch.no_grad():
                    output, loss, loss_stats = self.model_with_loss(batch)
            for k in avg_loss_stats:
                avg_loss_stats[k].update(loss_stats[k].mean().item(), batch["input"].size(0))
            del output, loss, loss_stats
        ret = {k: v.avg for k, v in avg_loss_stats.items()}
        ret["time"] = (time.time() - start) / 60.0
        return ret, results

    @torch.no_grad()
    def val(self, data_loader, gt, gt3d=None, smpl_model=None):
        """The reference's val() (trainer.py:326-328, save_result :456-469, datasets/coco_hp.py:92-138) for multi_pose: the detector path
        (network with the heads as trained, decode with opt.K, post-process) over the loader, then COCO's keypoint and box evaluation of
        the collected records on the device (coco_eval) -> (keypoint stats [10], bbox stats [12]); the two coco_eval.EvalResult are kept
        in self.last_val.  gt: coco_eval.GroundTruth.  A batch: dict(input [B,3,H,W], meta = dict(c [B,2], s [B], index [B] = the
        images' positions in gt)); images the loader never shows count as images without detections.
        gt3d (mesh_eval.GroundTruth3D, padded like gt) adds the 3D evaluation: the SMPL meshes of all K detection slots (smpl_model, or
        the one the trainer was built with; the `pose` and `shape` heads at the decode's centres, the exact blend shapes) are compared
        with the ground-truth person each detection's box matches (mesh_eval.MeshEvaluator), and the mesh_eval.MeshEvalResult (mpjpe,
        pa_mpjpe, pve, pa_pve, coverage in .extra) is kept in self.last_val['mesh'].  The return value does not change."""
        from . import coco_eval, decode
        from .detector import multi_pose_post_process
        opt = self.opt
        self._before_val()
        if _opt(opt, "task", "multi_pose") != "multi_pose":
            raise ValueError("HeadsTrainer.val: task %r not defined" % (_opt(opt, "task", None),))
        model = self.model
        meshes = None
        if gt3d is not None:
            from . import mesh_eval, smpl
            smpl_model = smpl_model if smpl_model is not None else self.smpl_model
            want = {"pose": 72, "shape": 10}
            if any(model.heads.get(h) != c for h, c in want.items()):
                raise ValueError("HeadsTrainer.val: the 3D evaluation needs the heads %s, the model has %s" % (want, dict(model.heads)))
            if smpl_model is None:
                raise ValueError("HeadsTrainer.val: the 3D evaluation needs an smpl_model")
            meshes = mesh_eval.MeshEvaluator(gt, gt3d)
        was_training = model.training
        model.eval()
        model.set_compute_dtype(model.compute_dtype)        # drops the cached plan: it is rebuilt from the parameters as they are now
        num_iters = _opt(opt, "num_iters", -1)
        if num_iters < 0:
            num_iters = len(data_loader)
        device = _opt(opt, "device", None)
        collected = coco_eval.CocoEvaluator(gt, "keypoints")
        for iter_id, batch in enumerate(data_loader):
            if iter_id >= num_iters:
                break
            x, meta = batch["input"], batch["meta"]
            if device is not None:
                x = x.to(device=device, non_blocking=True)
            out = model(x)[-1]
            dets, aux = decode.multi_pose_decode_logits(
                out["hm"], out["wh"], out["hps"], reg=out.get("reg") if _opt(opt, "reg_offset", True) else None,
                hm_hp=out.get("hm_hp") if _opt(opt, "hm_hp", True) else None,
                hp_offset=out.get("hp_offset") if _opt(opt, "reg_hp_offset", True) else None, K=_opt(opt, "K", 100), return_aux=True)
            results = multi_pose_post_process(dets, meta["c"], meta["s"], out["hm"].shape[2], out["hm"].shape[3])
            collected.update(meta["index"], results)
            if meshes is not None:
                verts, joints = smpl.lbs_from_heads(smpl_model, out["pose"].float().contiguous(), out["shape"].float().contiguous(),
                                                    aux["inds"], aux["inds"].shape[1], return_joints=True, exact=True)
                meshes.update(meta["index"], results, joints, verts)
        model.train(was_training)
        self.last_val = {"keypoints": collected.compute("keypoints"), "bbox": collected.compute("bbox")}
        if meshes is not None:
            self.last_val["mesh"] = meshes.compute()
        return self.last_val["keypoints"].stats, self.last_val["bbox"].stats

    def _before_val(self):
        """What val() does before it runs `self.model` (nothing here: the heads are the model's own parameters)."""

    def end_epoch(self, epoch):
        """The learning-rate drop of trainer.py:316-320; -> the new rate, or None when `epoch` is no step."""
        if epoch not in self.lr_step:
            return None
        lr = self.lr * (0.1 ** (self.lr_step.index(epoch) + 1))
        for param_group in self.optimizer.param_groups:
            param_group["lr"] = lr
        return lr

    def save_model(self, path, epoch):
        checkpoint.save_model(path, epoch, self.heads, self.optimizer)

    def load_model(self, model_path, resume=False):
        """-> start_epoch (trainer.py:167-169)."""
        _, _, start_epoch = checkpoint.load_model(self.heads, model_path, self.optimizer, resume, self.lr, self.lr_step)
        return start_epoch


class NetworkTrainer(HeadsTrainer):
    """HeadsTrainer with the whole network under autograd: `self.heads` is a train_model.TrainableDLASeg (the reference's graph on the
    trainable operators), Adam runs over all of its parameters (optim.Adam launches them in blocks of H3D_ADAM_CAPACITY tensors), and
    val() first loads the trained weights back into `model` (TrainableDLASeg.sync).
    bn: "frozen" (BatchNorm folded: frozen statistics) or "batch" (the reference's training-mode BatchNorm: run_epoch's
    model_with_loss.train(train) switches between batch and running statistics); None takes opt.bn if present, else "frozen"."""

    MODULE = TrainableDLASeg

    def __init__(self, opt, model, smpl_model=None, kp_regressor=None, bn=None):
        self.bn = _opt(opt, "bn", "frozen") if bn is None else bn
        super().__init__(opt, model, smpl_model, kp_regressor)

    def _build_module(self, model):
        return self.MODULE(model, bn=self.bn)

    def _before_val(self):
        self.heads.sync()
