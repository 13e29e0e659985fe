"""`python main_train.py --arch resnet18 --dataset cifar10 --lr 0.1 --epochs 182 --save_dir out` — pre-training of the
model the unlearning scripts start from; same flags and the same files as the reference's Classification/main_train.py:

    {save_dir}/0checkpoint.pth.tar      after every epoch: result, epoch, state_dict, best_sa, optimizer, scheduler
    {save_dir}/0model_SA_best.pth.tar   a copy whenever the validation accuracy improved
    {save_dir}/0net_train.png           the two accuracy curves (when matplotlib is present)

`optimizer` is stored in torch.optim.SGD.state_dict() layout (trainer/train.py: sgd_state_dict), so a checkpoint of
either code base resumes in the other with `--resume --checkpoint PATH`; `state_dict` is what `--model_path` of
generate_mask.py / main_random.py / main_forget.py loads.

The step runs on the HIP path: MFMA convolutions, fused BatchNorm, the fused classifier head K23 and the flat-arena
SGD.  `--library_conv` keeps the library convolutions, BatchNorm and head.  One deliberate difference: with `--seed S`
epoch e draws its shuffle and augmentation from seed S + e, so that a resumed run repeats the uninterrupted one bit
for bit (the reference seeds once and cannot).
"""
import os
import sys
import time

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import unlearn_saliency_amd.Classification  # noqa: F401
    __package__ = "unlearn_saliency_amd.Classification"

import numpy as np
import torch
import torch.nn as nn

from . import arg_parser, utils
from .trainer import get_optimizer_and_scheduler, train, validate
from .trainer.train import load_sgd_state_dict, sgd_state_dict

CHECKPOINT_KEYS = ("result", "epoch", "state_dict", "best_sa", "optimizer", "scheduler")


def _seed_epoch(seed, epoch):
    if seed:
        torch.manual_seed(seed + epoch)
        torch.cuda.manual_seed_all(seed + epoch)


def main(argv=None):
    args = arg_parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("pre-training needs a ROCm device: the fused kernels have no CPU fallback")
    torch.cuda.set_device(int(args.gpu))
    device = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(args.save_dir, exist_ok=True)
    if args.seed:
        utils.setup_seed(args.seed)

    model, train_loader, val_loader, test_loader, marked_loader = utils.setup_model_dataset(args)
    model.to(device)
    if not args.library_conv:
        from ..conv import use_salun_convs
        use_salun_convs(model)
        from ..norm import use_fused_bn
        use_fused_bn(model)
        from ..cls_head import use_fused_head
        use_fused_head(model)
    for loader in (train_loader, val_loader):
        loader.device = device

    print(f"number of train dataset {len(train_loader.dataset)}")
    print(f"number of val dataset {len(val_loader.dataset)}")

    criterion = nn.CrossEntropyLoss()
    best_sa = 0
    state = 0
    checkpoint = None
    if args.resume:
        print("resume from checkpoint {}".format(args.checkpoint))
        checkpoint = torch.load(args.checkpoint, map_location=device, weights_only=False)
        model.load_state_dict(checkpoint["state_dict"], strict=False)  # before the parameters move into the flat arena
    optimizer, scheduler = get_optimizer_and_scheduler(model, args)
    if checkpoint is not None:
        best_sa = checkpoint["best_sa"]
        start_epoch = checkpoint["epoch"]
        all_result = checkpoint["result"]
        load_sgd_state_dict(optimizer, checkpoint["optimizer"])
        scheduler.load_state_dict(checkpoint["scheduler"])
        print("loading from epoch: ", start_epoch, "best_sa=", best_sa)
    else:
        all_result = {"train_ta": [], "test_ta": [], "val_ta": []}
        start_epoch = 0

    try:
        for epoch in range(start_epoch, args.epochs):
            start_time = time.time()
            _seed_epoch(args.seed, epoch)
            print("Epoch #{}, Learning rate: {}".format(epoch, optimizer.param_groups[0]["lr"]))
            acc = train(train_loader, model, criterion, optimizer, epoch, args)
            tacc = validate(val_loader, model, criterion, args)
            scheduler.step()

            all_result["train_ta"].append(acc)
            all_result["val_ta"].append(tacc)
            is_best_sa = tacc > best_sa
            best_sa = max(tacc, best_sa)
            utils.save_checkpoint(
                {"result": all_result, "epoch": epoch + 1, "state_dict": model.state_dict(), "best_sa": best_sa,
                 "optimizer": sgd_state_dict(optimizer), "scheduler": scheduler.state_dict()},
                is_SA_best=is_best_sa, pruning=state, save_path=args.save_dir)
            print("one epoch duration:{}".format(time.time() - start_time))
    finally:
        optimizer.close()

    from .unlearn.impl import plot_training_curve
    plot_training_curve({"train": all_result["train_ta"], "val": all_result["val_ta"]}, args.save_dir, str(state) + "net")

    print("Performance on the test data set")
    validate(val_loader, model, criterion, args)
    if len(all_result["val_ta"]) != 0:
        val_pick_best_epoch = int(np.argmax(np.array(all_result["val_ta"])))
        print("* best SA = {}, Epoch = {}".format(all_result["val_ta"][val_pick_best_epoch], val_pick_best_epoch + 1))
    return all_result


if __name__ == "__main__":
    main()
