#!/usr/bin/env python3
"""The loop of the reference's examples/pointnet_classification.jl on the device:

    loss(x, y) = crossentropy(m(x), y);  opt = Flux.ADAM(lr)
    for epoch, batch:  gs = gradient(ps) do ... end;  Flux.update!(opt, ps, gs);  accuracy on the validation set

Every step is one replay of a captured graph (fx.TrainStepGraph: training-mode forward, cross-entropy, gradient, ADAM update,
running statistics, the dropout draw); the host only refills the batch and reads the loss once per epoch.

  python examples/pointnet_classification.py [--data DIR] [--epochs 5] [--batch 32] [--npoints 1024] [--lr 1e-3]

With --data (a directory holding ModelNet10, as flux3d_jl_amd.datasets.ModelNet10 takes it) the clouds are sampled from the meshes'
surfaces; without it a synthetic two-class set is used: points on a sphere against points in a flat disc.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flux3d_jl_amd as fx  # noqa: E402


def synthetic(count, npoints, seed):
    """(X (3, npoints, count) Float32, labels (count,)): class 0 on the unit sphere, class 1 in a disc of thickness 0.02."""
    rng = np.random.default_rng(seed)
    X, y = np.zeros((3, npoints, count), np.float32, order="F"), np.arange(count) % 2
    for b in range(count):
        pts = rng.standard_normal((3, npoints))
        if y[b] == 0:
            pts /= np.linalg.norm(pts, axis=0)
        else:
            pts[2] *= 0.02
        X[:, :, b] = pts
    return X, y


def modelnet10(root, train, npoints, limit):
    """The split's meshes as clouds of ``npoints`` points sampled on their surfaces and normalised, labels 0-based."""
    from flux3d_jl_amd import datasets
    d = datasets.ModelNet10(root, train=train)
    pick = np.random.default_rng(0).permutation(len(d))[:limit]
    X, y = np.zeros((3, npoints, len(pick)), np.float32, order="F"), np.zeros(len(pick), np.int64)
    for k, i in enumerate(pick):
        mesh, cls, _ = d[int(i)]
        pts = fx.sample_points(fx.gpu(mesh), npoints, seed=int(i)).to_host()[:, :, 0]
        pts = pts - pts.mean(axis=1, keepdims=True)
        X[:, :, k], y[k] = pts / max(float(np.abs(pts).max()), 1e-12), cls - 1
    return X, y, len(d.categories)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoints", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--limit", type=int, default=512, help="clouds taken from each ModelNet10 split")
    a = ap.parse_args()
    if a.data:
        Xt, yt, nc = modelnet10(a.data, True, a.npoints, a.limit)
        Xv, yv, _ = modelnet10(a.data, False, a.npoints, a.limit)
    else:
        (Xt, yt), (Xv, yv), nc = synthetic(8 * a.batch, a.npoints, 1), synthetic(2 * a.batch, a.npoints, 2), 2
    B = a.batch
    batches = [slice(i, i + B) for i in range(0, Xt.shape[2] - B + 1, B)]
    model, opt = fx.PointNet(nc), fx.ADAM(a.lr)
    step = fx.TrainStepGraph(model, opt, Xt[:, :, batches[0]], yt[batches[0]])   # (runs the first batch once, eagerly)
    for epoch in range(a.epochs):
        order = np.random.default_rng(epoch).permutation(len(batches))
        for k in order:
            step.refill(Xt[:, :, batches[k]], yt[batches[k]])
            out = step.step()
        step.synchronize()
        correct = total = 0
        for i in range(0, Xv.shape[2] - B + 1, B):
            correct += model.evaluate(fx.gpu(np.asfortranarray(Xv[:, :, i:i + B])), yv[i:i + B]).correct
            total += B
        print(f"epoch {epoch + 1}: loss of the last batch {float(out):.4f}, validation accuracy {correct / max(total, 1):.3f}")


if __name__ == "__main__":
    main()
