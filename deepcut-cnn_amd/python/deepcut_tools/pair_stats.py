"""The pair-statistics file of a model (`joint_pairs_stats`, caffe.proto:1184): the regression edges of `next_pred` and the mean /
standard deviation their targets were normalised with (pose_data_layer.cpp:453-455, 768-802).  Text, whitespace-separated: blocks of
`# <name>`, `<rows> <cols>`, rows x cols numbers; edges are 1-based class ids in the file and 0-based joints everywhere else here.
No trained file ships with the reference (its prototxt names a path on the authors' machine): `write_pair_stats` makes one."""
import numpy as np


def read_pair_stats(path):
    """-> (edges int32 [E, 2] of 0-based (joint, next joint), mean float64 [E, 2], std float64 [E, 2]), parsed and checked by the
    library (dc_pair_stats_read): raises caffe.DeepcutError naming what is wrong with a malformed file."""
    import caffe

    return caffe.pair_stats_read(path)


def write_pair_stats(path, edges, mean, std):
    """edges [E, 2] 0-based joints, mean / std [E, 2] -> the text file `read_pair_stats` reads (numbers with 17 significant digits:
    float64 values survive the round trip exactly)."""
    e = np.asarray(edges).reshape(-1, 2)
    m, s = np.asarray(mean, np.float64).reshape(-1, 2), np.asarray(std, np.float64).reshape(-1, 2)
    if not (e.shape == m.shape == s.shape):
        raise ValueError("edges, mean and std must all be [E, 2], got %s, %s, %s" % (e.shape, m.shape, s.shape))
    with open(path, "w") as f:
        for name, mat, fmt in (("edges", e.astype(np.int64) + 1, "%d"), ("means", m, "%.17g"), ("std_devs", s, "%.17g")):
            f.write("# %s\n%d %d\n" % (name, mat.shape[0], mat.shape[1]))
            for row in mat:
                f.write(" ".join(fmt % v for v in row) + "\n")
