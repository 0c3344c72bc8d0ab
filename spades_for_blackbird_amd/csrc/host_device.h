// host_device.h -- BBK_HOST_DEVICE: marks the helpers that a kernel and plain host C++ share (msd_bucket_tail.h,
// edge_ops.h, pairinfo_host.hpp), so that a stand-alone program can build them with g++ alone.  No includes.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BBK_HOST_DEVICE __host__ __device__
#else
#define BBK_HOST_DEVICE
#endif
