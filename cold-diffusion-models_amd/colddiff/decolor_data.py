"""The torchvision-backed datasets of the decolorization package (decolor-diffusion/diffusion/get_dataset.py, diffusion.py:493-535):
`Trainer(torchvision_dataset=True)` reads CIFAR-10 / CelebA / Flowers102 through torchvision's dataset classes, `Trainer(random_aug=True)`
adds RandomResizedCrop + ColorJitter.  Both are host-side PIL pipelines; torchvision is imported when one of them is asked for, and a
missing torchvision is an ImportError that names the option.  The default chain (CenterCrop, ToTensor, t * 2 - 1) does not come through
here: it is a `data.Recipe` on the device image cache."""
from pathlib import Path

from torch.utils import data

_SIZES = (('cifar10', (32, 32)), ('celebA', (128, 128)), ('flower', (128, 128)))


def _torchvision(option):
    try:
        import torchvision
    except ImportError as e:
        raise ImportError(f"{option} needs torchvision, which is not installed") from e
    return torchvision


def get_image_size(name):
    """(H, W) the reference's scripts train a dataset at; None for a name they do not know."""
    for key, size in _SIZES:
        if key in name:
            return size
    return None


def get_transform(image_size, random_aug=False, resize=False):
    T = _torchvision("get_transform (random_aug / torchvision_dataset)").transforms
    to_pm1 = [T.ToTensor(), T.Lambda(lambda t: (t * 2) - 1)]
    if image_size[0] == 64:
        return T.Compose([T.CenterCrop((128, 128)), T.Resize(image_size)] + to_pm1)
    if not random_aug:
        head = [T.Resize(image_size)] if resize else []
        return T.Compose(head + [T.CenterCrop(image_size)] + to_pm1)
    jitter = T.ColorJitter(0.8, 0.8, 0.8, 0.2)
    return T.Compose([T.RandomResizedCrop(size=image_size), T.RandomHorizontalFlip(), T.RandomApply([jitter], p=0.8)] + to_pm1)


def get_dataset(name, folder, image_size, random_aug=False):
    ds = _torchvision(f"get_dataset({name!r}) (Trainer(torchvision_dataset=True))").datasets
    print(folder)
    tf = lambda resize=False: get_transform(image_size, random_aug=random_aug, resize=resize)
    table = {
        'cifar10_train': lambda: ds.CIFAR10(folder, train=True, transform=tf()),
        'cifar10_test': lambda: ds.CIFAR10(folder, train=False, transform=tf()),
        'CelebA_train': lambda: ds.CelebA(folder, split='train', transform=tf(), download=True),
        'CelebA_test': lambda: ds.CelebA(folder, split='test', transform=tf()),
        'flower_train': lambda: ds.Flowers102(folder, split='train', transform=tf(True), download=True),
        'flower_test': lambda: ds.Flowers102(folder, split='test', transform=tf(True), download=True),
    }
    return table[name]() if name in table else None


class FolderDataset(data.Dataset):
    """An image folder through the random-augmentation chain (`Trainer(random_aug=True)`)."""

    def __init__(self, folder, image_size, exts=('jpg', 'jpeg', 'png'), random_aug=False):
        super().__init__()
        self.folder, self.image_size = folder, image_size
        self.paths = [p for ext in exts for p in Path(f'{folder}').glob(f'**/*.{ext}')]
        self.transform = get_transform(image_size, random_aug=random_aug)

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, index):
        from PIL import Image
        return self.transform(Image.open(self.paths[index]))
