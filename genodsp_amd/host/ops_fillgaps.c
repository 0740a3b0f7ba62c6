/* ops_fillgaps.c -- fillgaps (device shim).  Not an operator of the reference: the bases at which the signal is unknown --
 * not above a threshold, or zero -- take their values from the known bases around them, by a line between the two, or
 * from the nearer, the left or the right one.  Everything else in the table treats a zero as a measurement; this says
 * "the value here is unknown".  The threshold is given as `segments` takes it (ops_segments.c parses it for both).
 * The definition is at gdsp_fillgaps (include/genodsp_hip.h).
 *
 * The driver finds this operator through opgroup_fillgaps, at the end of this file (host_services.h); every call into the
 * device library for it stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_fillgaps)

typedef struct dspop_fillgaps
	{
	dspop   common;
	segments_opts o;                                               /* the threshold and its ties; nothing else of it is used */
	int     known;                                                 /* GDSP_FILL_KNOWN_* */
	int     how;                                                   /* GDSP_FILL_LINEAR .. */
	int     ends;                                                  /* GDSP_FILL_ENDS_* */
	u32     maxGap;                                                /* 0: none */
	} dspop_fillgaps;

OP_SHORT (op_fillgaps, "fill the bases not above a threshold from the known bases around them (not in genodsp)")

void op_fillgaps_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sTreat every base whose value is not above a threshold as unknown, and give it a value taken\n", indent);
	fprintf (f, "%sfrom the nearest known base on either side: by default the line between the two. Known bases\n", indent);
	fprintf (f, "%skeep their values. A chromosome without a known base is left as it is. `= fillgaps\n", indent);
	fprintf (f, "%s--maxgap=1K = smooth W=101` smooths a track without dragging every window that meets a short\n", indent);
	fprintf (f, "%suncovered stretch towards zero. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s [<threshold>] [options]\n", indent, name);
	fprintf (f, "%s  <threshold>              numeric threshold (default 0.0)\n", indent);
	fprintf (f, "%s  --threshold=<variable>   (T=) threshold from a named variable, e.g. percentile99\n", indent);
	fprintf (f, "%s  --ties:below|above       whether values equal to the threshold count as below (default) or above\n", indent);
	fprintf (f, "%s  --known=above            a base is known when its value is above the threshold\n", indent);
	fprintf (f, "%s                           (this is the default)\n", indent);
	fprintf (f, "%s  --known=nonzero          a base is known when its value is neither zero nor NaN; negative\n", indent);
	fprintf (f, "%s                           values count, and no threshold may be given\n", indent);
	fprintf (f, "%s  --as=linear              the line between the known bases before and behind the gap\n", indent);
	fprintf (f, "%s                           (this is the default)\n", indent);
	fprintf (f, "%s  --as=nearest             the value of the nearer of the two; halfway, of the one before\n", indent);
	fprintf (f, "%s  --as=left                the value of the known base before the gap (forward fill)\n", indent);
	fprintf (f, "%s  --as=right               the value of the known base behind the gap\n", indent);
	fprintf (f, "%s  --ends=extend            where the side that is asked for does not exist, as in the gaps at a\n", indent);
	fprintf (f, "%s                           chromosome's ends, take the value of the side that does\n", indent);
	fprintf (f, "%s                           (this is the default)\n", indent);
	fprintf (f, "%s  --ends=keep              leave such bases as they are\n", indent);
	fprintf (f, "%s  --maxgap=<bases>         leave gaps of more than this many bases as they are (e.g. 10K)\n", indent);
	}

dspop* op_fillgaps_parse (char* name, int argc, char** argv)
	{
	dspop_fillgaps* op = (dspop_fillgaps*) new_op (name, sizeof(dspop_fillgaps), false);
	segments_opts_init (&op->o);
	op->known = GDSP_FILL_KNOWN_ABOVE;
	op->how   = GDSP_FILL_LINEAR;
	op->ends  = GDSP_FILL_ENDS_EXTEND;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (segments_threshold_take (&op->o, name, arg)) continue;
		if (strcmp_prefix (arg, "--known=") == 0)
			{
			if      (strcmp (argVal, "above")   == 0) op->known = GDSP_FILL_KNOWN_ABOVE;
			else if (strcmp (argVal, "nonzero") == 0) op->known = GDSP_FILL_KNOWN_NONZERO;
			else chastise ("[%s] --known must be above or nonzero (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp_prefix (arg, "--as=") == 0)
			{
			if      (strcmp (argVal, "linear")  == 0) op->how = GDSP_FILL_LINEAR;
			else if (strcmp (argVal, "nearest") == 0) op->how = GDSP_FILL_NEAREST;
			else if (strcmp (argVal, "left")    == 0) op->how = GDSP_FILL_LEFT;
			else if (strcmp (argVal, "right")   == 0) op->how = GDSP_FILL_RIGHT;
			else chastise ("[%s] --as must be linear, nearest, left or right (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp_prefix (arg, "--ends=") == 0)
			{
			if      (strcmp (argVal, "extend") == 0) op->ends = GDSP_FILL_ENDS_EXTEND;
			else if (strcmp (argVal, "keep")   == 0) op->ends = GDSP_FILL_ENDS_KEEP;
			else chastise ("[%s] --ends must be extend or keep (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp_prefix (arg, "--maxgap=") == 0)
			{
			int r = string_to_unitized_int (argVal, /*thousands*/ true);
			if (r == 0) chastise ("[%s] --maxgap can't be zero (\"%s\")\n", name, arg);
			if (r < 0)  chastise ("[%s] --maxgap can't be negative (\"%s\")\n", name, arg);
			op->maxGap = (u32) r;
			continue;
			}
		segments_opts_take_other (&op->o, name, arg);              /* --debug, an option nobody knows, the threshold */
		}
	if ((op->known == GDSP_FILL_KNOWN_NONZERO) && op->o.haveThreshold)
		chastise ("[%s] --known=nonzero takes no threshold\n", name);
	return (dspop*) op;
	}

void op_fillgaps_free (dspop* _op)
	{
	dspop_fillgaps* op = (dspop_fillgaps*) _op;
	segments_opts_free (&op->o);
	free (op);
	}

/* the variable is fetched when the operator first runs: by then `percentile` or `stats` has set it */
static void resolve_threshold (dspop_fillgaps* op)
	{
	if (op->known == GDSP_FILL_KNOWN_NONZERO) return;
	resolve_variable (&op->common, &op->o.thresholdVarName, &op->o.threshold, "threshold");
	if (op->o.threshold != op->o.threshold)
		{ fprintf (stderr, "[%s] the threshold is not a number\n", op->common.name);  exit (EXIT_FAILURE); }
	}

void op_fillgaps_apply (dspop* _op, arg_dont_complain(char* vName), u32 vLen, valtype* v)
	{
	dspop_fillgaps* op = (dspop_fillgaps*) _op;
	resolve_threshold (op);
	check_gdsp (gdsp_fillgaps (v, vLen, op->o.threshold, op->o.tiesAbove, op->known, op->how, op->ends, op->maxGap, op_stream ()),
	            _op->name);
	}

/* the driver: without --maxgap a base depends on its whole chromosome (a gap may be as long as that), which then stays in
 * one piece under --sharding=bases.  With --maxgap=G a stretch that sees G+1 bases to either side of its own computes its
 * own bases as the whole chromosome would:
 *   - a gap of at most G bases has both its neighbours (or the chromosome's end, which the stretch then ends at too) within
 *     G of each of its bases, so the stretch sees the gap whole, with what bounds it, and fills it as the chromosome does;
 *   - a longer gap that meets the stretch's own bases shows to it either whole, as a gap of more than G bases, or cut
 *     by the stretch's end: then it runs from one of the stretch's own bases through the G+1 bases of the halo, an end run
 *     of at least G+2 bases.  Either way it is longer than G and is left alone, as the chromosome leaves it.
 * One launch sequence per device */
static int fillgaps_reach (dspop* _op, u32* left, u32* right)
	{
	dspop_fillgaps* op = (dspop_fillgaps*) _op;
	if (op->maxGap == 0) return false;
	*left = *right = op->maxGap + 1;
	return true;
	}

static int fillgaps_batch (dspop* _op, const gdsp_batch_item* items, int nitems, void* stream)
	{
	dspop_fillgaps* op = (dspop_fillgaps*) _op;
	resolve_threshold (op);
	return gdsp_fillgaps_batch (items, nitems, op->o.threshold, op->o.tiesAbove, op->known, op->how, op->ends, op->maxGap, stream);
	}

static const dspinfo fillgapsRows[] =
	{ dspinforecord("fillgaps", op_fillgaps), dspinfoalias ("fill_gaps"), dspinfoalias ("interpolate"), dspinfoalias ("impute") };
static const optraits fillgapsTraits[] = { { op_fillgaps_apply, true, false, fillgaps_reach, fillgaps_batch, NULL } };
const opgroup opgroup_fillgaps = OPGROUP (fillgapsRows, fillgapsTraits, NULL);
