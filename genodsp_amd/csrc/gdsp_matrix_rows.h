// gdsp_matrix_rows.h -- the host half the matrix operators share (gdsp_matrixover.hip: matrixover; gdsp_regionsover.hip:
// regionsover): the template argument a figure stands for, and the rows of one device end to end -- the launches of as
// many rows as the device's buffers take, the way of each launch's rows back to the sources that own them, and the cells
// the kernel left on its to-do list, which are finished through gdsp_interval_stats_batch.  What a row is made of (a
// position and a code word; a start, an end and a code word), which kernel runs and which interval of its chromosome a
// cell is stay with the two files.  Nothing here is reached from a kernel.
#pragma once
#include <math.h>
#include <type_traits>
#include "gdsp_anchors.h"
#include "gdsp_matrix_cell.h"

// f (std::integral_constant<int, WHAT> ()) for the figure `what` (checked: one of GDSP_MATRIX_*)
template <typename F>
static inline void mx_with_figure (int what, F f)
	{
	switch (what)
		{
		case GDSP_MATRIX_MEAN:  f (std::integral_constant<int, GDSP_MATRIX_MEAN> ());   break;
		case GDSP_MATRIX_SUM:   f (std::integral_constant<int, GDSP_MATRIX_SUM> ());    break;
		case GDSP_MATRIX_COUNT: f (std::integral_constant<int, GDSP_MATRIX_COUNT> ());  break;
		case GDSP_MATRIX_MIN:   f (std::integral_constant<int, GDSP_MATRIX_MIN> ());    break;
		default:                f (std::integral_constant<int, GDSP_MATRIX_MAX> ());    break;
		}
	}

// the figure of a cell the exact interval call computed
static inline double mx_figure_of (const gdsp_interval_stat& st, int what)
	{
	switch (what)
		{
		case GDSP_MATRIX_MEAN:  return st.mean;
		case GDSP_MATRIX_SUM:   return st.sum;
		case GDSP_MATRIX_COUNT: return (double) st.count;
		case GDSP_MATRIX_MIN:   return st.min;
		default:                return st.max;
		}
	}

// All rows of the current device (at least one, at most 2^32 - 1), ncols cells each, into h_rows.  items: the device's
// vectors, item k being source mine[k], which owns the rows first[k] .. first[k+1] - 1 and gets them at h_rows[mine[k]].
// cols[0 .. C): what describes the rows, one u32 of each per row; they are uploaded one behind the other, so column c
// of the rows from r0 on begins at d_cols + c * na + r0 (na: all rows).  maxRows: the most rows of a launch, 0 for as
// many as MX_LAUNCH_CELLS cells.  last: the call's counters; [2] counts the cells finished here, [3] the launches.
// who, rowsName: the entry point and what it calls its rows, as the complaints name them.
//   launch (d_cols + r0, na, nr, d_out, d_todo, d_ntodo, s, launches) -> GDSP_OK or an error: the kernel over nr rows
//   interval (a, j, n, &gLo, &gHi): cell j of row a, in a vector of n values, as its bases [gLo, gHi); gLo >= gHi: none
template <size_t C, typename Launch, typename Interval>
static int mx_rows_on_device (const std::vector<gdsp_batch_item>& items, const std::vector<uint64_t>& first, const int* mine,
                              const std::vector<uint32_t> (&cols)[C], uint32_t ncols, int what, double lo, double hi,
                              double* const* h_rows, uint32_t maxRows, uint64_t* last, void* stream, const char* who,
                              const char* rowsName, Launch launch, Interval interval)
	{
	const int      nmine = (int) items.size ();
	const uint64_t na    = first[nmine];
	hipStream_t s = gdsp_stream (stream);

	uint64_t perLaunch = std::max<uint64_t> (1, MX_LAUNCH_CELLS / ncols);
	if (maxRows != 0) perLaunch = std::min<uint64_t> (perLaunch, maxRows);
	perLaunch = std::min (perLaunch, na);
	const size_t cells = (size_t) perLaunch * ncols;

	GdspAnchorHeld held;
	uint32_t *d_cols = NULL, *d_todo = NULL;
	double*   d_out = NULL;
	int rc = held.alloc ((void**) &d_cols, C * na * sizeof(uint32_t), who, rowsName);
	if (rc == GDSP_OK) rc = held.alloc ((void**) &d_out, cells * sizeof(double), who, "rows");
	if (rc == GDSP_OK) rc = held.alloc ((void**) &d_todo, (cells + 1) * sizeof(uint32_t), who, "to-do list");     // the counter, then the list
	if (rc != GDSP_OK) return rc;
	for (size_t c=0 ; c<C ; c++)
		GDSP_HIP_TRY (hipMemcpyAsync (d_cols + c * na, cols[c].data (), na * sizeof(uint32_t), hipMemcpyHostToDevice, s));

	std::vector<uint32_t> todo, tVec, tStart, tEnd;
	std::vector<double*>  tWhere;
	std::vector<gdsp_interval_stat> tStat;
	for (uint64_t r0=0 ; r0<na ; r0+=perLaunch)
		{
		const uint32_t nr = (uint32_t) std::min<uint64_t> (perLaunch, na - r0);
		uint32_t ntodo = 0;
		GDSP_HIP_TRY (hipMemsetAsync (d_todo, 0, sizeof(uint32_t), s));
		rc = launch (d_cols + r0, na, nr, d_out, d_todo + 1, d_todo, s, &last[3]);
		if (rc != GDSP_OK) return rc;
		GDSP_HIP_TRY (hipMemcpyAsync (&ntodo, d_todo, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		// the rows, to the sources that own them
		int k = (int) (std::upper_bound (first.begin (), first.end (), r0) - first.begin ()) - 1;
		for (uint64_t a=r0 ; a<r0+nr ; )
			{
			while (first[k+1] <= a) k++;
			const uint64_t b = std::min<uint64_t> (first[k+1], r0 + nr);
			GDSP_HIP_TRY (hipMemcpyAsync (h_rows[mine[k]] + (size_t) (a - first[k]) * ncols, d_out + (size_t) (a - r0) * ncols,
			                              (size_t) (b - a) * ncols * sizeof(double), hipMemcpyDeviceToHost, s));
			a = b;
			}
		GDSP_HIP_TRY (hipStreamSynchronize (s));
		if (ntodo == 0) continue;

		// the cells the device left: each is one interval of its chromosome, computed by the exact interval call
		if (ntodo > (uint64_t) nr * ncols) return gdsp_anchor_refuse (who, "the to-do list is longer than the launch");
		todo.resize (ntodo);
		GDSP_HIP_TRY (hipMemcpyAsync (todo.data (), d_todo + 1, (size_t) ntodo * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		GDSP_HIP_TRY (hipStreamSynchronize (s));
		tVec.clear ();  tStart.clear ();  tEnd.clear ();  tWhere.clear ();
		for (uint32_t t=0 ; t<ntodo ; t++)
			{
			const uint64_t a = r0 + todo[t] / ncols;
			const uint32_t j = todo[t] % ncols;
			const int kk = (int) (std::upper_bound (first.begin (), first.end (), a) - first.begin ()) - 1;
			int64_t gLo, gHi;
			interval (a, j, (int64_t) items[kk].n, &gLo, &gHi);
			double* where = h_rows[mine[kk]] + (size_t) (a - first[kk]) * ncols + j;
			if (gLo >= gHi) { *where = ((what == GDSP_MATRIX_COUNT) || (what == GDSP_MATRIX_SUM))? 0.0 : NAN;  continue; }
			tVec.push_back ((uint32_t) kk);  tStart.push_back ((uint32_t) gLo);  tEnd.push_back ((uint32_t) gHi);
			tWhere.push_back (where);
			}
		tStat.resize (tWhere.size ());
		rc = gdsp_interval_stats_batch (items.data (), nmine, tVec.data (), tStart.data (), tEnd.data (), (uint32_t) tWhere.size (),
		                                lo, hi, tStat.data (), (void*) s);
		if (rc != GDSP_OK) return rc;
		for (size_t t=0 ; t<tWhere.size () ; t++) *tWhere[t] = mx_figure_of (tStat[t], what);
		last[2] += ntodo;
		}
	return GDSP_OK;
	}
