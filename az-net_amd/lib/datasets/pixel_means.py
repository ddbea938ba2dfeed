"""Pixel means of a dataset, in BGR order (the reference's tools/pixel_means.py:45-61).

The reference keeps a running mean, rescaled at every image; here every channel is summed exactly in uint64 over all
images and divided once.  Host NumPy on purpose: the cost is the image decode, and a kernel would move 0.5 MB per image
to the device to save a 0.3 ms sum ("Proposal diagnosis")."""
import numpy as np


def channel_sums(imdb):
    """(sums uint64 [3] in BGR order, number of pixels) over every image of the imdb, printing the reference's progress
    line every 1000 images and at the end."""
    from detect.test import _prefetched
    num_images = len(imdb.image_index)
    sums = np.zeros((3,), dtype=np.uint64)
    num_pixels = 0
    images = _prefetched(imdb, list(range(num_images)), depth=2)
    for i in range(num_images):
        im = np.asarray(next(images))
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError("pixel_means: image %d is %s %s, not uint8 HxWx3" % (i, im.dtype, im.shape))
        sums += im.reshape(-1, 3).sum(axis=0, dtype=np.uint64)
        num_pixels += im.shape[0] * im.shape[1]
        if i % 1000 == 0 or i == num_images - 1:
            print('Processing {}/{}, the mean is ({})'.format(i, num_images, sums / float(num_pixels)))
    return sums, num_pixels


def pixel_means(imdb):
    """BGR means float64 [3] of all pixels of the imdb (zeros for an empty one)."""
    sums, num_pixels = channel_sums(imdb)
    if num_pixels == 0:
        return np.zeros((3,))
    return sums / float(num_pixels)
