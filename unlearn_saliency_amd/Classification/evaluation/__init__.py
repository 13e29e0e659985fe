"""SVC membership-inference attack used for the "MIA" column (reference
Classification/evaluation/SVC_MIA.py:85-150).  backend="sklearn" (default): the reference's CPU evaluation;
backend="device" (`--mia device`): probabilities, features, fit and predict on the device (K25, ops_svc.py)."""
from .svc_mia import BACKENDS, SVC_MIA
