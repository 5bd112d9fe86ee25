"""run.py --mode train --hierarchical on the GPU: the training loop with the fine pass runs end to end,
writes the final checkpoint, and what it logs and saves as loss / PSNR is the fine pass's."""
import math
import os

import pytest
import torch

import run as cli


@pytest.mark.gpu
def test_train_mode_hierarchical_writes_a_checkpoint_with_the_fine_psnr(tmp_path, monkeypatch):
    from nerfmi import train
    monkeypatch.chdir(tmp_path)
    fine = []
    step = train.Trainer.step

    def recording_step(self, *a, **kw):
        out = step(self, *a, **kw)
        assert self.hierarchical and self.n_importance == self.config.num_importance
        fine.append(float(self.loss_parts[0]))
        return out

    monkeypatch.setattr(train.Trainer, "step", recording_step)
    assert cli.main(["--mode", "train", "--hierarchical", "--random_init", "0", "--iterations", "6"]) == 0
    assert "checkpoint_final.pt" in os.listdir(tmp_path / "checkpoints")
    assert len(fine) == 6 and train.train_nerf.losses == fine            # the fine MSE, not the summed loss
    assert train.train_nerf.psnrs == [-10.0 * math.log10(v) for v in fine]
    ck = torch.load(tmp_path / "checkpoints" / "checkpoint_final.pt", map_location="cpu", weights_only=True)
    assert ck["iteration"] == 6 and ck["loss"] == fine[-1] and ck["psnr"] == -10.0 * math.log10(fine[-1])
