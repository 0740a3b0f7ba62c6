// gdsp_anchors.hip -- what of gdsp_anchors.h the library holds once: the check on the device that every anchor lies inside
// its vector, which is all that stands between a bad position and a kernel that reads outside its vector.
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

int gdsp_anchor_check (const gdsp_batch_item* items, int nitems, const uint32_t* d_pos, const uint32_t* d_code, uint32_t count,
                       hipStream_t s, const char* who)
	{
	std::vector<uint32_t> h_n (nitems);
	for (int i=0 ; i<nitems ; i++) h_n[i] = items[i].n;
	uint32_t* d_work = NULL;                                    // the flag, then the lengths
	if (hipMalloc ((void**) &d_work, (size_t) (nitems + 1) * sizeof(uint32_t)) != hipSuccess)
		{ gdsp_set_error ("%s: no device memory for the anchor check", who);  return GDSP_ENOMEM; }
	uint32_t bad = 0;
	hipError_t e = hipMemsetAsync (d_work, 0, sizeof(uint32_t), s);
	if (e == hipSuccess) e = hipMemcpyAsync (d_work + 1, h_n.data (), (size_t) nitems * sizeof(uint32_t), hipMemcpyHostToDevice, s);
	if (e == hipSuccess) e = hipStreamSynchronize (s);           // (h_n is pageable: the copy has left it)
	if (e == hipSuccess)
		{
		uint32_t g = (count + 255) / 256;
		if (g > 1024) g = 1024;                                  // (a thread strides over the anchors beyond 1024 x 256)
		hipLaunchKernelGGL (anchor_check_kernel, dim3 (g), dim3 (256), 0, s, d_pos, d_code, count, d_work + 1, (uint32_t) nitems, d_work);
		e = hipGetLastError ();
		}
	if (e == hipSuccess) e = hipMemcpyAsync (&bad, d_work, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
	if (e == hipSuccess) e = hipStreamSynchronize (s);
	(void) hipFree (d_work);
	GDSP_HIP_TRY (e);
	return (bad == 0)? GDSP_OK : gdsp_anchor_refuse (who, "an anchor lies outside its vector");
	}
