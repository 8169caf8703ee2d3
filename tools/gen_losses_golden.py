"""Regenerates tests/golden/losses_ref.npz: the reference's own `models.losses` classes and `models.utils._sigmoid`, imported and run on
the CPU in fp32, on the inputs of tests/losses_ref.py's builders -- per case the inputs, the loss value and `autograd.grad` with respect
to the head tensor.  tests/test_oracle_losses.py holds the restatement of tests/losses_ref.py against this file.

`trains/trainer.py` cannot be imported (it pulls in cv2 through the debugger), so the file pins the five loss classes; the task-level
weighting is checked against the restatement.  Usage: python tools/gen_losses_golden.py [reference src/lib directory]"""
import os
import sys
import warnings

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src/lib"
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import losses_ref as R  # noqa: E402

from models import losses as ref_losses  # noqa: E402   (reference)
from models import utils as ref_utils  # noqa: E402    (reference)

OUT = os.path.join(ROOT, "tests", "golden", "losses_ref.npz")

# name -> (class, builder arguments); shared with tests/test_oracle_losses.py through the file's keys
FOCAL_CASES = {"focal_some": (11, (2, 2, 8, 12), "some"), "focal_none": (12, (2, 2, 8, 12), "none"), "focal_all": (13, (1, 1, 3, 5), "all")}
REG_CASES = {"RegL1Loss_u8": ("RegL1Loss", 21, 3, 2, 32, torch.uint8), "RegL1Loss_f32": ("RegL1Loss", 22, 3, 2, 32, torch.float32),
             "RegWeightedL1Loss_f32": ("RegWeightedL1Loss", 23, 1, 34, 32, torch.float32),
             "RegWeightedL1Loss_u8": ("RegWeightedL1Loss", 29, 1, 2, 1, torch.uint8),
             "NormRegL1Loss_u8": ("NormRegL1Loss", 25, 3, 2, 32, torch.uint8), "RegLoss_u8": ("RegLoss", 26, 3, 2, 32, torch.uint8),
             "RegLoss_f32": ("RegLoss", 27, 1, 1, 32, torch.float32)}
H, W = 8, 12


def main():
    warnings.simplefilter("ignore")
    out = {}
    for name, (seed, shape, positives) in FOCAL_CASES.items():
        x, gt = R.focal_inputs(seed, shape, positives)
        # from the logits, as every call site of the reference does (trainer.py:93-94); _sigmoid works in place: feed it a non-leaf
        leaf = x.clone().requires_grad_(True)
        pred = ref_utils._sigmoid(leaf * 1.0)
        loss = ref_losses.FocalLoss()(pred, gt)
        g, = torch.autograd.grad(loss, leaf)
        # and FocalLoss alone, on the probabilities
        p_leaf = pred.detach().clone().requires_grad_(True)
        loss_p = ref_losses.FocalLoss()(p_leaf, gt)
        gp, = torch.autograd.grad(loss_p, p_leaf)
        out.update({name + ".x": x.numpy(), name + ".gt": gt.numpy(), name + ".pred": pred.detach().numpy(), name + ".loss": loss.detach().numpy(),
                    name + ".grad_x": g.numpy(), name + ".loss_p": loss_p.detach().numpy(), name + ".grad_p": gp.numpy()})
    for name, (cls, seed, B, C, M, mdt) in REG_CASES.items():
        feat, mask, ind, target = R.reg_inputs(seed, cls, B, C, M, H, W, mdt)
        leaf = feat.clone().requires_grad_(True)
        loss = getattr(ref_losses, cls)()(leaf, mask, ind, target)
        g, = torch.autograd.grad(loss, leaf)
        assert float(g.abs().max()) > 0, name
        out.update({name + ".feat": feat.numpy(), name + ".mask": mask.numpy(), name + ".ind": ind.numpy(), name + ".target": target.numpy(),
                    name + ".loss": loss.detach().numpy(), name + ".grad": g.numpy()})
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
