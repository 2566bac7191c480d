from colddiff.decolor_data import get_dataset, get_image_size, get_transform

__all__ = ["get_dataset", "get_image_size", "get_transform"]
