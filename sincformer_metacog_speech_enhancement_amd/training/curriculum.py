"""Host-side mirror of training/curriculum.py (CurriculumScheduler :18-105): which SNR levels, targets and objective an
epoch trains with.  Pure host logic; the stage lengths come from config.CURRICULUM_STAGE{1,2,3}_EPOCHS."""
from .. import config

_ALL_SNRS = [-5, 0, 5, 10]


class CurriculumScheduler:
    def __init__(self):
        self.stage1_epochs = config.CURRICULUM_STAGE1_EPOCHS
        self.stage2_epochs = config.CURRICULUM_STAGE2_EPOCHS
        self.stage3_epochs = config.CURRICULUM_STAGE3_EPOCHS
        self.total_epochs = self.stage1_epochs + self.stage2_epochs + self.stage3_epochs

    def _stage_of(self, epoch):
        if epoch < self.stage1_epochs:
            return 1
        return 2 if epoch < self.stage1_epochs + self.stage2_epochs else 3

    def get_stage(self, epoch):
        """epoch (0-based) -> dict(stage, snr_levels, use_vq, use_soft_mask, loss_type, description)"""
        stage = self._stage_of(epoch)
        if stage == 1:
            snrs, loss, text = [5, 10], "mse", "Stage 1: High-SNR + soft mask only"
        elif stage == 2:
            # the first third of the stage leaves -5 dB out
            progress = (epoch - self.stage1_epochs) / self.stage2_epochs
            snrs = [0, 5, 10] if progress < 0.33 else list(_ALL_SNRS)
            loss, text = "mse+perceptual", "Stage 2: Progressive low-SNR (SNRs=%s)" % (snrs,)
        else:
            snrs, loss, text = list(_ALL_SNRS), "perceptual+vq+adversarial", "Stage 3: VQ activation + intelligibility loss"
        return {"stage": stage, "snr_levels": snrs, "use_vq": stage == 3, "use_soft_mask": stage != 3, "loss_type": loss,
                "description": text}

    def print_schedule(self):
        """one block per stage: its epochs, SNR levels at its first epoch, VQ switch and objective"""
        lengths = [self.stage1_epochs, self.stage2_epochs, self.stage3_epochs]
        print("=" * 60)
        print("Curriculum Learning Schedule")
        print("=" * 60)
        first = 0
        for n in lengths:
            if n > 0:
                info = self.get_stage(first)
                print("\n--- %s ---" % info["description"])
                print("  Epochs: %d - %d" % (first, first + n - 1))
                print("  SNR levels: %s" % (info["snr_levels"],))
                print("  VQ active: %s" % info["use_vq"])
                print("  Loss: %s" % info["loss_type"])
            first += n
