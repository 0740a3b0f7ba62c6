// gdsp_anchors.hip -- what of gdsp_anchors.h the library holds once: the checks on the device that every anchor, and every
// region, lies inside its vector, which is all that stands between a bad position and a kernel that reads outside its vector.
#include "gdsp_anchors.h"

// *d_bad = 1 when some anchor names a vector the call does not have or a position outside its vector
__global__ void anchor_check_kernel (const uint32_t* __restrict__ d_pos, const uint32_t* __restrict__ d_code, uint32_t count,
                                     const uint32_t* __restrict__ d_n, uint32_t nvec, uint32_t* __restrict__ d_bad)
	{
	bool bad = false;
	for (uint32_t i=blockIdx.x*blockDim.x+threadIdx.x ; i<count ; i+=gridDim.x*blockDim.x)
		{
		const uint32_t vec = gdsp_anchor_vec (d_code[i]);
		bad |= (vec >= nvec) || (d_pos[i] >= d_n[(vec < nvec)? vec : 0]);
		}
	if (bad) atomicOr (d_bad, 1u);
	}

// *d_bad = 1 when some region names a vector the call does not have or is not s < e <= n of its vector
__global__ void region_check_kernel (const uint32_t* __restrict__ d_start, const uint32_t* __restrict__ d_end,
                                     const uint32_t* __restrict__ d_code, uint32_t count, const uint32_t* __restrict__ d_n,
                                     uint32_t nvec, uint32_t* __restrict__ d_bad)
	{
	bool bad = false;
	for (uint32_t i=blockIdx.x*blockDim.x+threadIdx.x ; i<count ; i+=gridDim.x*blockDim.x)
		{
		const uint32_t vec = gdsp_anchor_vec (d_code[i]);
		bad |= (vec >= nvec) || (d_start[i] >= d_end[i]) || (d_end[i] > d_n[(vec < nvec)? vec : 0]);
		}
	if (bad) atomicOr (d_bad, 1u);
	}

// the host half of both: launch (grid, block, d_n, d_bad) starts the kernel on s over the items' lengths d_n[0 .. nitems)
// and the cleared flag *d_bad; noMemory, verdict: the complaints, as the two callers word them
template <typename Launch>
static int check_on_device (const gdsp_batch_item* items, int nitems, uint32_t count, hipStream_t s, const char* who,
                            const char* noMemory, const char* verdict, Launch launch)
	{
	std::vector<uint32_t> h_n (nitems);
	for (int i=0 ; i<nitems ; i++) h_n[i] = items[i].n;
	uint32_t* d_work = NULL;                                    // the flag, then the lengths
	if (hipMalloc ((void**) &d_work, (size_t) (nitems + 1) * sizeof(uint32_t)) != hipSuccess)
		{ gdsp_set_error ("%s: %s", who, noMemory);  return GDSP_ENOMEM; }
	uint32_t bad = 0;
	hipError_t e = hipMemsetAsync (d_work, 0, sizeof(uint32_t), s);
	if (e == hipSuccess) e = hipMemcpyAsync (d_work + 1, h_n.data (), (size_t) nitems * sizeof(uint32_t), hipMemcpyHostToDevice, s);
	if (e == hipSuccess) e = hipStreamSynchronize (s);           // (h_n is pageable: the copy has left it)
	if (e == hipSuccess)
		{
		uint32_t g = (count + 255) / 256;
		if (g > 1024) g = 1024;                                  // (a thread strides over what lies beyond 1024 x 256)
		launch (dim3 (g), dim3 (256), d_work + 1, d_work);
		e = hipGetLastError ();
		}
	if (e == hipSuccess) e = hipMemcpyAsync (&bad, d_work, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
	if (e == hipSuccess) e = hipStreamSynchronize (s);
	(void) hipFree (d_work);
	GDSP_HIP_TRY (e);
	return (bad == 0)? GDSP_OK : gdsp_anchor_refuse (who, verdict);
	}

int gdsp_anchor_check (const gdsp_batch_item* items, int nitems, const uint32_t* d_pos, const uint32_t* d_code, uint32_t count,
                       hipStream_t s, const char* who)
	{
	return check_on_device (items, nitems, count, s, who, "no device memory for the anchor check", "an anchor lies outside its vector",
		[&] (dim3 grid, dim3 block, const uint32_t* d_n, uint32_t* d_bad)
			{ hipLaunchKernelGGL (anchor_check_kernel, grid, block, 0, s, d_pos, d_code, count, d_n, (uint32_t) nitems, d_bad); });
	}

int gdsp_region_check (const gdsp_batch_item* items, int nitems, const uint32_t* d_start, const uint32_t* d_end, const uint32_t* d_code,
                       uint32_t count, hipStream_t s, const char* who)
	{
	return check_on_device (items, nitems, count, s, who, "no device memory for the region check", "a region is empty or lies outside its vector",
		[&] (dim3 grid, dim3 block, const uint32_t* d_n, uint32_t* d_bad)
			{ hipLaunchKernelGGL (region_check_kernel, grid, block, 0, s, d_start, d_end, d_code, count, d_n, (uint32_t) nitems, d_bad); });
	}
