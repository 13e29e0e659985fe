"""Golden vectors for K25 (RBF C-SVC fit / predict on the device): sklearn.svm.SVC(C=3, gamma="auto", kernel="rbf")
on small membership-style feature sets, and the reference's `evaluation.SVC_MIA` on the end-to-end fixture.

    python tests/golden/make_golden_svc.py

Per case: X, y, Q (float32), sklearn's dual_coef_ / support_ / intercept_ / decision_function(Q) at tol=1e-7
(`dec_ref`), gap = max|dec(tol=1e-3) - dec(tol=1e-7)| of sklearn against itself, the bound b = 4 * max(gap, 1e-3)
(1e-3: the stopping tolerance both solvers use; 4: margin for a different working-set path inside the same
eps-optimal set) and the fraction of queries with |dec_ref| <= b, which must be <= 0.03 (else the case's seed moves on).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

C = 3.0
NQ = 300
SIZES = ((2, 2), (64, 64), (257, 257), (1024, 1024))
UNBALANCED = (100, 37)
FRAC_CAP = 0.03


def conf1d(r, n, member):
    return r.beta(20.0 if member else 6.0, 1.0, size=(n, 1))


def prob10d(r, n, member):
    conc = np.full((n, 10), 0.3)
    conc[np.arange(n), r.integers(0, 10, n)] = 30.0 if member else 8.0
    g = r.gamma(conc)
    return g / g.sum(1, keepdims=True)


def binary(r, n, member):
    return (r.random((n, 1)) < (0.95 if member else 0.8)).astype(np.float64)


FAMILIES = dict(conf1d=conf1d, prob10d=prob10d, binary=binary)


def sk_fit(X, y, tol):
    from sklearn.svm import SVC
    return SVC(C=C, gamma="auto", kernel="rbf", tol=tol).fit(X.astype(np.float64), y)


def record(X, y, Q):
    """sklearn's answers for one training set and query set, with the bound derived from sklearn against itself."""
    tight, loose = sk_fit(X, y, 1e-7), sk_fit(X, y, 1e-3)
    Q64 = Q.astype(np.float64)
    dec_ref = tight.decision_function(Q64)
    gap = float(np.abs(loose.decision_function(Q64) - dec_ref).max())
    b = 4.0 * max(gap, 1e-3)
    frac = float((np.abs(dec_ref) <= b).mean())
    return dict(dual_coef=tight.dual_coef_[0].astype(np.float64), support=tight.support_.astype(np.int64),
                intercept=np.float64(tight.intercept_[0]), dec_ref=dec_ref.astype(np.float64), gap=np.float64(gap),
                b=np.float64(b), frac=np.float64(frac), pred_ref=tight.predict(Q64).astype(np.uint8))


def make_case(family, n_in, n_out, seed):
    gen = FAMILIES[family]
    while True:
        r = np.random.default_rng(seed)
        X = np.concatenate([gen(r, n_in, True), gen(r, n_out, False)]).astype(np.float32)
        y = np.concatenate([np.ones(n_in), np.zeros(n_out)]).astype(np.uint8)
        Q = np.concatenate([gen(r, NQ, True), gen(r, NQ, False)]).astype(np.float32)
        if len(np.unique(X[y == 1], axis=0)) + len(np.unique(X[y == 0], axis=0)) >= 2 and np.isfinite(X).all():
            rec = record(X, y, Q)
            if rec["frac"] <= FRAC_CAP:
                return dict(X=X, y=y, Q=Q, seed=np.int64(seed), **rec)
        seed += 1000


def end_to_end():
    """The five attack accuracies of the reference's SVC_MIA on the eval fixture, and sklearn's decisions on the
    target points per feature (features computed by this package's own expressions on the host)."""
    import types
    import make_golden as MG
    from fixtures import TinyCNN, eval_loaders, tiny_state
    from unlearn_saliency_amd.Classification.evaluation import svc_mia
    MG.import_reference_classification()
    stub = types.ModuleType("imagenet")
    stub.get_x_y_from_data_dict = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError())
    sys.modules["imagenet"] = stub
    ref = MG._load("ref_svc_mia", MG.REF + "/Classification/evaluation/SVC_MIA.py")
    model = TinyCNN()
    model.load_state_dict(tiny_state(21))
    ld = eval_loaders()
    m = ref.SVC_MIA(shadow_train=ld["shadow_train"], shadow_test=ld["shadow_test"], target_train=None,
                    target_test=ld["target_test"], model=model)
    out = {"e2e_ref_" + k: np.float64(v) for k, v in m.items()}
    sets = {k: svc_mia._collect(l, model) for k, l in dict(st=ld["shadow_train"], so=ld["shadow_test"], tt=None,
                                                          to=ld["target_test"]).items()}
    for name, (s_in, s_out, _, t_out) in svc_mia.mia_features(sets).items():
        X = torch.cat([s_in, s_out]).numpy().reshape(len(s_in) + len(s_out), -1).astype(np.float32)
        y = np.concatenate([np.ones(len(s_in)), np.zeros(len(s_out))]).astype(np.uint8)
        Q = t_out.numpy().reshape(len(t_out), -1).astype(np.float32)
        rec = record(X, y, Q)
        assert abs((1 - rec["pred_ref"].mean()) - m[name]) < 1e-12, (name, rec["pred_ref"].mean(), m[name])
        for k in ("dec_ref", "gap", "b", "frac"):
            out[f"e2e_{k}_{name}"] = rec[k]
    return out


def main():
    out, names = {}, []
    for f, family in enumerate(FAMILIES):
        cases = list(SIZES) + ([UNBALANCED] if family == "conf1d" else [])
        for n_in, n_out in cases:
            name = f"{family}_{n_in}_{n_out}"
            case = make_case(family, n_in, n_out, 25_000 + 100 * f + n_in)
            names.append(name)
            for k, v in case.items():
                out[f"{name}/{k}"] = v
            print(f"{name}: seed {int(case['seed'])} n_sv {len(case['support'])} gap {float(case['gap']):.2e} "
                  f"b {float(case['b']):.2e} within-b {float(case['frac']):.4f}")
    out["cases"] = np.array(names)
    out.update(end_to_end())
    for k in sorted(out):
        if k.startswith("e2e_") and not k.startswith("e2e_dec"):
            print(k, float(out[k]))
    path = os.path.join(HERE, "svc_rbf.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
