"""Stand-in for the one name imported by the reference's SIFT module."""


def rgb_to_grayscale(image):
    return 0.299 * image[..., 0:1, :, :] + 0.587 * image[..., 1:2, :, :] + 0.114 * image[..., 2:3, :, :]
