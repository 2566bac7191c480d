"""Drop-in for the `diffusion` package of snowification/.  Like the decolorization package's (which it shares file for file upstream) it
lives one level down because of its generic name: put `cold-diffusion-models_amd/snowification` on sys.path (next to
`cold-diffusion-models_amd` itself) and the reference's `from diffusion import GaussianDiffusion, Trainer, get_dataset` /
`from diffusion.model.get_model import get_model` resolve here.  `GaussianDiffusion` takes forward_process_type 'Snow' and 'Decolorization'."""
from diffusion.diffusion import GaussianDiffusion, Trainer
from diffusion import get_dataset                       # noqa: F401  (the scripts read get_dataset.get_image_size)
from diffusion.forward_process_impl import DeColorization, Snow
from diffusion.model.unet_convnext import UnetConvNextBlock

__all__ = ["GaussianDiffusion", "Trainer", "Snow", "DeColorization", "UnetConvNextBlock", "get_dataset"]
