from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

BACKENDS = ("sklearn", "device")
SVC_C = 3.0     # the reference's SVC(C=3, gamma="auto", kernel="rbf"); sklearn's default tol
SVC_TOL = 1e-3


def _collect(loader, model, n_classes=10, on_device=False):
    dev = next(model.parameters()).device
    out = dev if on_device else torch.device("cpu")
    if loader is None:
        return torch.zeros([0, n_classes], device=out), torch.zeros([0], dtype=torch.int64, device=out)
    probs, labels = [], []
    model.eval()
    with torch.no_grad():
        for x, y in loader:
            probs.append(F.softmax(model(x.to(dev)), dim=-1).to(out))
            labels.append(y.to(out))
    return torch.cat(probs), torch.cat(labels)


def _entropy(p):
    return -torch.where(p > 0, p * p.log(), torch.zeros_like(p)).sum(-1)


def _m_entropy(p, labels):
    """Reference m_entropy (SVC_MIA.py:12-22) as written: the columns named by ANY label in the
    batch are swapped to (1-p, log p) for every row; both log terms are log p (floored)."""
    floor = torch.tensor(1e-30).log()
    logp = torch.where(p > 0, p.log(), floor)
    mod_p, mod_logp = p.clone(), logp.clone()
    cols = labels.long()
    mod_p[:, cols] = (1 - p)[:, cols]
    mod_logp[:, cols] = logp[:, cols]
    return -(mod_p * mod_logp).sum(-1)


def _svc_acc(shadow_in, shadow_out, target_in, target_out):
    from sklearn.svm import SVC
    X = torch.cat([shadow_in, shadow_out]).numpy().reshape(len(shadow_in) + len(shadow_out), -1)
    Y = np.concatenate([np.ones(len(shadow_in)), np.zeros(len(shadow_out))])
    clf = SVC(C=3, gamma="auto", kernel="rbf").fit(X, Y)
    accs = []
    if len(target_in):
        accs.append(clf.predict(target_in.numpy().reshape(len(target_in), -1)).mean())
    if len(target_out):
        accs.append(1 - clf.predict(target_out.numpy().reshape(len(target_out), -1)).mean())
    return float(np.mean(accs))


def _svc_acc_device(shadow_in, shadow_out, target_in, target_out, stages=None):
    """The same attack accuracy on K25 (csrc/salun_svc.hip): gram -> fit -> decision, all stream-ordered, then ONE
    host read (the two prediction means and the solver's status).  sklearn is not imported."""
    from ... import ops_svc
    n_in, n_out = len(shadow_in), len(shadow_out)
    if n_in == 0 or n_out == 0:
        raise ValueError("SVC_MIA: the shadow set needs members and non-members")
    dev = shadow_in.device
    X = torch.cat([shadow_in, shadow_out]).reshape(n_in + n_out, -1).float().contiguous()
    y = torch.cat([torch.ones(n_in, dtype=torch.uint8, device=dev), torch.zeros(n_out, dtype=torch.uint8, device=dev)])
    d = X.shape[1]
    Q = torch.cat([target_in.reshape(len(target_in), d), target_out.reshape(len(target_out), d)]).float().contiguous()
    m_in, m_out = len(target_in), len(target_out)
    if m_in + m_out == 0:
        raise ValueError("SVC_MIA: no target points")
    # the probability-vector feature has one entry per class: past K25's register-resident limit it takes the wide pair
    model = ops_svc.fit(X, y, C=SVC_C, eps=SVC_TOL, wait=False, stages=stages, wide=d > ops_svc.max_features(False))
    _, pred = ops_svc.decision(model, Q, stages=stages)
    p = pred.double()
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    host = torch.cat([torch.stack([p[:m_in].mean() if m_in else zero, p[m_in:].mean() if m_out else zero,
                                   torch.isfinite(X).all().double(), torch.isfinite(Q).all().double()]),
                      model.status.double()]).cpu()
    if not (host[2] and host[3]):
        raise ValueError("SVC_MIA: non-finite features")
    iterations = int(host[4])
    if not host[5]:  # the loop is bounded, so non-finite features end here too: reported above
        raise ops_svc.SvcNotConverged(iterations, model.max_iter)
    if stages is not None:
        stages.setdefault("iterations", []).append(iterations)
    accs = ([float(host[0])] if m_in else []) + ([1 - float(host[1])] if m_out else [])
    return float(np.mean(accs))


def mia_features(sets):
    """name -> [shadow-train, shadow-test, target-train, target-test] feature tensors from (probabilities, labels)."""
    def feat(fn):
        return [fn(*sets[k]).float() for k in ("st", "so", "tt", "to")]

    def like(p, *shape):
        return torch.zeros(*shape, device=p.device)

    features = {
        "correctness": lambda p, y: (p.argmax(1) == y).int() if len(p) else like(p, 0),
        "confidence": lambda p, y: p.gather(1, y[:, None].long()) if len(p) else like(p, 0, 1),
        "entropy": lambda p, y: _entropy(p),
        "m_entropy": lambda p, y: _m_entropy(p, y) if len(p) else like(p, 0),
        "prob": lambda p, y: p,
    }
    return {name: feat(fn) for name, fn in features.items()}


def SVC_MIA(shadow_train, target_train, target_test, shadow_test, model, backend="sklearn", stages=None):
    """dict(correctness, confidence, entropy, m_entropy, prob) of attack accuracies; the paper's
    MIA number is result['confidence'] * 100 with target_test = forget set.

    backend="sklearn" (default): probabilities to the host, sklearn.svm.SVC per feature.
    backend="device": probabilities, features, fit and predict stay on the model's device (K25); `stages`, if a
    dict, receives the device-synchronised seconds of collect / gram / fit / decision (tools/mia_bench.py)."""
    if backend not in BACKENDS:
        raise ValueError(f"SVC_MIA backend must be one of {BACKENDS}, got {backend!r}")
    device = backend == "device"
    if device and not next(model.parameters()).is_cuda:
        raise RuntimeError("SVC_MIA(backend='device') needs the model on a ROCm device; no CPU fallback")
    if stages is not None:
        import time
        torch.cuda.synchronize()
        t0 = time.perf_counter()
    sets = {k: _collect(l, model, on_device=device) for k, l in dict(st=shadow_train, so=shadow_test, tt=target_train,
                                                                      to=target_test).items()}
    if stages is not None:
        torch.cuda.synchronize()
        stages["collect"] = stages.get("collect", 0.0) + time.perf_counter() - t0
    if device:
        return {name: _svc_acc_device(*f, stages=stages) for name, f in mia_features(sets).items()}
    return {name: _svc_acc(*f) for name, f in mia_features(sets).items()}
