"""bench.py --dump-outputs without a GPU: which rows of the timed path's last step are written, in float32, and the
64 MB bound met by one fixed, seeded sample of envs shared by every per-env array."""
from types import SimpleNamespace

import numpy as np
import torch

import bench


def _fake_train_step(T, E, J, H, n_updates):
    st = {"reward": torch.arange(T * E, dtype=torch.float32).reshape(T, E, 1),
          "terminated": torch.zeros((T, E, 1), dtype=torch.bool),
          "actions_discrete": torch.arange(T * E * J, dtype=torch.int32).reshape(T, E, J, 1),
          "actions_continuous": torch.rand((T, E, J, 1)),
          "hidden_state": torch.randn((T + 1, E, J, H))}
    st["terminated"][T - 1] = True
    agent, mixer = torch.nn.Linear(3, 2), torch.nn.Linear(2, 1)
    updates = [torch.tensor([1.0, 2.0, 3.0, 4.0]) + i for i in range(n_updates - 1)]
    updates.append({"loss": torch.tensor(9.0), "grad_norm": torch.tensor(8.0), "eval_qtot_avg": torch.tensor(7.0),
                    "target_qtot_avg": torch.tensor(6.0)})
    step_fn = SimpleNamespace(runner=SimpleNamespace(stage=st), state={"updates": updates},
                              learner=SimpleNamespace(mac=SimpleNamespace(agent=agent), eval_qmix_net=mixer))
    return step_fn, st, agent


def test_dump_outputs_train_last_step_rows(tmp_path):
    T, E, J, H = 10, 6, 3, 4
    step_fn, st, agent = _fake_train_step(T, E, J, H, n_updates=3)
    out = bench.last_step_outputs("train", step_fn, steps=27, episode_limit=T)   # last step: row 6 of its episode batch
    bench.dump_outputs(str(tmp_path), out, E)
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["reward"], st["reward"][:7, :, 0].numpy())
    np.testing.assert_array_equal(got["actions_discrete"], st["actions_discrete"][:7, :, :, 0].numpy().astype(np.float32))
    np.testing.assert_array_equal(got["hidden_state"], st["hidden_state"][6].numpy())
    np.testing.assert_array_equal(got["update_stats"], [[1, 2, 3, 4], [2, 3, 4, 5], [9, 7, 6, 8]])
    np.testing.assert_array_equal(got["agent.weight"], agent.weight.detach().numpy())
    assert "mixer.bias" in got and "env_index" not in got
    # a whole last episode: every row of the batch
    out = bench.last_step_outputs("train", step_fn, steps=30, episode_limit=T)
    assert out["reward"][0].shape == (T, E)


def test_dump_outputs_bounded_by_a_seeded_env_sample(tmp_path, monkeypatch):
    T, E, J, H = 10, 64, 3, 4
    step_fn, st, _ = _fake_train_step(T, E, J, H, n_updates=1)
    out = bench.last_step_outputs("train", step_fn, steps=T, episode_limit=T)
    full = sum(t.numel() for t, _ in out.values()) * 4
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", full // 3)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), out, E)
    sizes = sum(p.stat().st_size for p in dirs[0].glob("*.npy"))
    assert sizes <= full // 3 + 128 * len(list(dirs[0].glob("*.npy")))   # (+ the .npy headers)
    idx = np.load(dirs[0] / "env_index.npy").astype(np.int64)
    assert 0 < len(idx) < E and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(idx, np.load(dirs[1] / "env_index.npy"))
    np.testing.assert_array_equal(np.load(dirs[0] / "reward.npy"), st["reward"][:, idx, 0].numpy())
    np.testing.assert_array_equal(np.load(dirs[0] / "hidden_state.npy"), st["hidden_state"][T - 1, idx].numpy())
    np.testing.assert_array_equal(np.load(dirs[0] / "update_stats.npy"), [[9, 7, 6, 8]])


def test_dump_outputs_env_mode(tmp_path):
    E, R = 5, 4
    track = torch.randint(0, 2, (R, E), dtype=torch.uint8)
    info = {"r_d": torch.rand(E), "r_p": torch.rand(E), "r_j": torch.rand(E), "radar_tracking": track.t(),
            "step_count": torch.full((E,), 3, dtype=torch.int32), "radar_pds": torch.rand(R, E).t(),
            "snr_with_jamming": torch.rand(R, E).t()}
    rew, ter = torch.rand(E), torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8).view(torch.bool)
    bench.dump_outputs(str(tmp_path), bench.last_step_outputs("env", SimpleNamespace(last=(rew, ter, info)), 7, 100), E)
    np.testing.assert_array_equal(np.load(tmp_path / "terminated.npy"), [0, 1, 0, 0, 1])
    np.testing.assert_array_equal(np.load(tmp_path / "radar_tracking.npy"), track.t().numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "r_dpj.npy")[:, 1], info["r_p"].numpy())
