"""Drop-in module name for MonoGS: ``from fused_ssim import fused_ssim``
(/root/reference/gaussian_splatting/utils/loss_utils.py:19, called at :43-45 with ``padding="valid"``)."""
from monogs_amd.ssim import fused_ssim  # noqa: F401
