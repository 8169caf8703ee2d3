"""h3d_amd -- MI355X (gfx950) native implementation of the multi_pose inference hot path of
Aaron20127/human-3d-reconstruction: DLA-34 + DCNv2 forward, heat-map decode, SMPL/LBS.

Host side is Python on PyTorch-ROCm (device memory, streams, torch.distributed only); all
compute goes through the C-ABI library `csrc/libh3d_hip.so` (include/h3d.h).  There is no CPU
fallback: using a compute entry point without the built library raises.

Reference-named entry points (same names / argument meaning as the reference's src/lib):
    models.model.dla_net                      -> h3d_amd.model.dla_net
    models.DCNv2.dcn_v2.{dcn_v2_conv,DCNv2,DCN,dcn_v2_pooling,DCNv2Pooling,DCNPooling},
        _ext.{dcn_v2_forward,dcn_v2_psroi_pooling_forward} -> h3d_amd.dcn_v2.*
    training (opt-in; the names above stay inference-only): _ext.{dcn_v2_backward,dcn_v2_psroi_pooling_backward} -> h3d_amd.dcn_v2.*,
        _DCNv2.apply / _DCNv2Pooling.apply -> h3d_amd.dcn_v2.{dcn_v2_conv_autograd,dcn_v2_pooling_autograd}, DCNv2 / DCN / DCNv2Pooling /
        DCNPooling under autograd -> h3d_amd.dcn_v2.{TrainableDCNv2,TrainableDCN,TrainableDCNv2Pooling,TrainableDCNPooling}
    models.decode.{_nms,_topk,_topk_channel,multi_pose_decode,ctdet_decode} -> h3d_amd.decode.*
    models.utils.{_sigmoid,_gather_feat,_transpose_and_gather_feat} -> h3d_amd.utils.*
    utils.post_process.multi_pose_post_process -> h3d_amd.detector.multi_pose_post_process
    models.losses.{FocalLoss,RegL1Loss,RegLoss,NormRegL1Loss,RegWeightedL1Loss},
        trains.trainer.{loss_multi_pose,loss_obj_detection} -> h3d_amd.losses.*
    datasets.coco_hp.COCOHP.{_get_label,_get_dataset}, the label block of datasets.coco.COCO.__getitem__,
        utils.image.get_affine_transform -> h3d_amd.targets.{multi_pose_targets,ctdet_targets,get_affine_transform}
    datasets.coco_hp.COCOHP.{_get_input (train branch),__getitem__}, datasets.coco.COCO.__getitem__ (split == 'train'),
        utils.image.color_aug -> h3d_amd.train_input.{draw_params,train_input,multi_pose_train_batch,ctdet_train_batch}
Training the heads `Conv3x3 + ReLU + Conv1x1` (models.model.DLASeg.__init__ / forward) on the frozen backbone:
        h3d_amd.heads.{heads_autograd,TrainableHeads}
    torch.optim.Adam as trains.trainer.HMRTrainer uses it, HMRModelWithLoss / run_epoch / the lr_step drop, save_model / load_model
        with the optimiser state -> h3d_amd.optim.Adam, h3d_amd.trainer.HeadsTrainer, h3d_amd.checkpoint.{save_model,load_model}
Training plain convolutions (nn.Conv2d, models.model.BasicBlock / Root with folded BatchNorm) -> h3d_amd.conv.{conv2d_backward,
        conv2d_autograd,TrainableConv2d,TrainableBasicBlock}
Training the whole DLA-34 (models.model.DLASeg with frozen BatchNorm statistics): nn.MaxPool2d(2, 2) and IDAUp's depthwise
        ConvTranspose2d + skip add -> h3d_amd.pool_up.{max_pool2_backward,upsample_backward,max_pool2_autograd,up_add_autograd};
        the network under autograd -> h3d_amd.train_model.TrainableDLASeg, h3d_amd.trainer.NetworkTrainer
Without a counterpart in the reference: the 3D evaluation of the SMPL output, MPJPE / PA-MPJPE / PVE / PA-PVE on the device
        -> h3d_amd.mesh_eval.{GroundTruth3D,pointset_errors,metric_means,evaluate_pairs,MeshEvaluator}, HeadsTrainer.val(loader, gt, gt3d, smpl_model)
"""
from . import synth  # noqa: F401

__all__ = ["synth", "arch", "model", "engine", "weights", "plan", "dcn_calibrate", "decode", "utils", "dcn_v2", "smpl", "detector", "losses", "targets", "heads", "train_input", "optim", "trainer", "checkpoint", "mesh_eval", "conv", "pool_up", "bn", "train_model"]
