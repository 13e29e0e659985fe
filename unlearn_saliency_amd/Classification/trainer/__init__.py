"""The pre-training epoch and the evaluation loop used for the UA/RA/TA accuracies.  (The reference's trainer package
also exports a `train_with_rewind` that does not exist upstream; it is not reproduced.)"""
from .train import get_optimizer_and_scheduler, train
from .val import validate
