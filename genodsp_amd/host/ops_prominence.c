/* ops_prominence.c -- prominence (device shim).  Not an operator of the reference: how far every base stands above its
 * surroundings inside a window, the measure behind scipy.signal.peak_prominences and MATLAB's MinPeakProminence.
 * Window, centring and edge rule are bestmax's (ops_minmax.c, minmax.c:1527-1603 / :1616-1640 in the reference).
 * The definition is at gdsp_prominence (include/genodsp_hip.h).
 *
 * The driver finds this operator through opgroup_prominence, at the end of this file (host_services.h); every call into the
 * device library for it stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_prominence)

typedef struct dspop_prominence { dspop common;  u32 windowSize;  int what; } dspop_prominence;

OP_SHORT (op_prominence, "how far each base stands above its surroundings (not in genodsp)")

void op_prominence_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sReplace every base by its topographic prominence inside the window centred on it.\n", indent);
	fprintf (f, "%sFrom base i, with value x, walk left while the bases are inside the window and the\n", indent);
	fprintf (f, "%schromosome and not greater than x, and note the smallest value met (x if none);\n", indent);
	fprintf (f, "%swalk right likewise. The base level is the larger of the two minima, and the\n", indent);
	fprintf (f, "%sprominence is x minus the base level: 0 for a base with a higher neighbour or at a\n", indent);
	fprintf (f, "%schromosome end, the same for every base of a plateau, never negative. For an odd\n", indent);
	fprintf (f, "%swindow this is scipy.signal.peak_prominences with wlen=<length>. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s [options]\n", indent, name);
	fprintf (f, "%s  --window=<length>        (W=) window size (default: global window, else 100; at most %d);\n",
	         indent, GDSP_PROMINENCE_MAX_WINDOW);
	fprintf (f, "%s                           (W-1)/2 bases to the left, the rest to the right\n", indent);
	fprintf (f, "%s  --as=prominence          write the prominence (this is the default)\n", indent);
	fprintf (f, "%s  --as=base                write the base level instead: the local background\n", indent);
	}

dspop* op_prominence_parse (char* name, int argc, char** argv)
	{
	dspop_prominence* op = (dspop_prominence*) new_op (name, sizeof(dspop_prominence), false);
	op->windowSize = (u32) get_named_global ("windowSize", 100);
	op->what       = GDSP_PROMINENCE_VALUE;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (is_opt3 (arg, "window", "W")) { op->windowSize = window_arg (name, arg, argVal, "window size");  continue; }
		if (strcmp_prefix (arg, "--as=") == 0)
			{
			if      (strcmp (argVal, "prominence") == 0) op->what = GDSP_PROMINENCE_VALUE;
			else if (strcmp (argVal, "base")       == 0) op->what = GDSP_PROMINENCE_BASE;
			else chastise ("[%s] --as must be prominence or base (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp (arg, "--debug") == 0) continue;
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->windowSize > GDSP_PROMINENCE_MAX_WINDOW)
		chastise ("[%s] window size %u is above the largest this operator supports (%d)\n",
		          name, op->windowSize, GDSP_PROMINENCE_MAX_WINDOW);
	return (dspop*) op;
	}

void op_prominence_free (dspop* op) { free (op); }

void op_prominence_apply (dspop* _op, char* vName, u32 vLen, valtype* v)
	{
	dspop_prominence* op = (dspop_prominence*) _op;
	check_gdsp (gdsp_prominence (v, partner_vector (vName), vLen, op->windowSize, op->what, op_stream ()), _op->name);
	flip_vector (vName);
	}

/* the driver: bestmax's window (neither walk leaves [i-wL, i+wR]), and one launch per device (windows above the maximum
 * were refused at parse time) */
static int prominence_reach (dspop* op, u32* left, u32* right) { return reach_centred (((dspop_prominence*) op)->windowSize, left, right); }

static int prominence_batch (dspop* _op, const gdsp_batch_item* items, int nitems, void* stream)
	{
	dspop_prominence* op = (dspop_prominence*) _op;
	return gdsp_prominence_batch (items, nitems, op->windowSize, op->what, stream);
	}

static const dspinfo  prominenceRows[]   = { dspinforecord("prominence", op_prominence), dspinfoalias ("peakprominence") };
static const optraits prominenceTraits[] = { { op_prominence_apply, false, false, prominence_reach, prominence_batch, NULL } };
const opgroup opgroup_prominence = OPGROUP (prominenceRows, prominenceTraits, NULL);
