"""Drop-in for the `diffusion` package of decolor-diffusion/ (the colourization experiment).  `diffusion` is too generic a name for the
shared package root, so -- like the defading-generation package -- it lives one level down: put
`cold-diffusion-models_amd/decolor_diffusion` on sys.path (next to `cold-diffusion-models_amd` itself) and the reference's
`from diffusion import GaussianDiffusion, Trainer, get_dataset` / `from diffusion.model.get_model import get_model` resolve here."""
from diffusion.diffusion import GaussianDiffusion, Trainer
from diffusion import get_dataset                       # noqa: F401  (the scripts read get_dataset.get_image_size)
from diffusion.forward_process_impl import DeColorization
from diffusion.model.unet_convnext import UnetConvNextBlock

__all__ = ["GaussianDiffusion", "Trainer", "DeColorization", "UnetConvNextBlock", "get_dataset"]
