"""Writes tests/golden/dscnn_leftover_max_map.npy: one feature map [1, 1, 99, 10] for which, under the golden signal-preserving
weights (e2e_golden.npz, he.blob), the largest output of DS-CNN block 1 AND of block 2 lies in the block's K-split leftover tile
(positions 120..140 of the 47 x 3 plane, 240..244 of the 49 x 5 plane), each more than twice the rest of its plane.
tests/test_dscnn_leftover_combine_gpu.py asserts both on the oracle before it uses the map.

Found by gradient ascent on the CPU oracle (oracle/dscnn.py): Adam on the map, clamped to the range of the golden random maps,
maximising the log ratio of a soft maximum over the leftover positions to one over the rest of the plane.  Four starts; the best
is kept.  CPU only, a few seconds per start.

    python tests/golden/make_leftover_max_map.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import dscnn as o_dscnn  # noqa: E402


def main():
    g = np.load(os.path.join(HERE, "e2e_golden.npz"))
    blob, state, off = g["he.blob"], {}, 0
    for k, shp in o_dscnn.state_shapes(12).items():
        n = int(np.prod(shp))
        state[k] = torch.from_numpy(blob[off:off + n].reshape(shp).copy())
        off += n
    lim = float(np.abs(g["x_rand"]).max())

    def planes(x):
        _, layers = o_dscnn.forward(state, x, return_layers=True)
        return (layers["dsconv1"][:, :, 1:-1, 1:-1].reshape(1, 64, -1), layers["dsconv2"][:, :, 1:-1, 1:-1].reshape(1, 64, -1))

    def soft_max(v, t=0.05):
        return t * torch.logsumexp(v.reshape(-1) / t, 0)

    best = None
    for seed in range(4):
        torch.manual_seed(seed)
        x = (torch.randn(1, 1, 99, 10) * 2).requires_grad_(True)
        opt = torch.optim.Adam([x], lr=0.2)
        for _ in range(400):
            opt.zero_grad()
            z1, z2 = planes(x)
            gain2 = torch.log(soft_max(z2[:, :, 240:]) + 1e-6) - torch.log(soft_max(z2[:, :, :240]) + 1e-6)
            gain1 = torch.log(soft_max(z1[:, :, 120:]) + 1e-6) - torch.log(soft_max(z1[:, :, :120]) + 1e-6)
            (-gain2 - 0.5 * torch.clamp(gain1, max=1.2)).backward()
            opt.step()
            with torch.no_grad():
                x.clamp_(-lim, lim)
        with torch.no_grad():
            xf = x.detach().float()
            z1, z2 = planes(xf)
            r1 = float(z1[:, :, 120:].max() / z1[:, :, :120].max())
            r2 = float(z2[:, :, 240:].max() / z2[:, :, :240].max())
        print(f"start {seed}: leftover maximum / rest of the plane: block 1 {r1:.3f}, block 2 {r2:.3f}")
        if best is None or min(r1, r2) > best[0]:
            best = (min(r1, r2), xf.numpy().astype(np.float32))
    assert best[0] > 2.0
    np.save(os.path.join(HERE, "dscnn_leftover_max_map.npy"), best[1])


if __name__ == "__main__":
    main()
