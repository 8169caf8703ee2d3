"""Checkpoint interchange with the reference trainer (trains/trainer.py:475-539):
`torch.load(path)['state_dict']`, optional 'module.' prefix from DataParallel, shape mismatch
or missing keys keep the model's own initialisation (strict=False), as the reference does.  With an optimiser the checkpoint also holds
its state_dict under 'optimizer', and `resume` restores it with the learning rate the reference's schedule has reached
(trains/trainer.py:511-539)."""
import torch


def load_model(model, model_path, optimizer=None, resume=False, lr=None, lr_step=None):
    """-> model; with an optimiser (model, optimizer, start_epoch), start_epoch = the checkpoint's epoch when its optimiser state was
    resumed, else 0."""
    start_epoch = 0
    ck = torch.load(model_path, map_location="cpu", weights_only=False)
    print("loaded {}, epoch {}".format(model_path, ck.get("epoch", "?")))
    src = ck["state_dict"] if "state_dict" in ck else ck
    sd = {(k[7:] if k.startswith("module") and not k.startswith("module_list") else k): v for k, v in src.items()}
    own = model.state_dict()
    for k in list(sd):
        if k in own:
            if tuple(sd[k].shape) != tuple(own[k].shape):
                print("Skip loading parameter {}, required shape{}, loaded shape{}.".format(
                    k, tuple(own[k].shape), tuple(sd[k].shape)))
                sd[k] = own[k]
        else:
            print("Drop parameter {}.".format(k))
            del sd[k]
    for k in own:
        if k not in sd:
            print("No param {}.".format(k))
            sd[k] = own[k]
    model.load_state_dict(sd, strict=False)
    if optimizer is not None and resume:
        if "optimizer" in ck:
            optimizer.load_state_dict(ck["optimizer"])
            start_epoch = ck["epoch"]
            start_lr = lr
            for step in lr_step:
                if start_epoch >= step:
                    start_lr *= 0.1
            for param_group in optimizer.param_groups:
                param_group["lr"] = start_lr
            print("Resumed optimizer with start lr", start_lr)
        else:
            print("No optimizer parameters in checkpoint.")
    if optimizer is not None:
        return model, optimizer, start_epoch
    return model


def save_model(path, epoch, model, optimizer=None):
    data = {"epoch": epoch, "state_dict": model.state_dict()}
    if optimizer is not None:
        data["optimizer"] = optimizer.state_dict()
    torch.save(data, path)
