/* ops_localcorrelate.c -- localcorrelate (device shim).  Not an operator of the reference: where along the genome do the
 * signal and a second track agree -- replicate against replicate, treatment against control, plus strand against minus
 * strand.  correlate (ops_correlate.c) answers that for the genome as a whole and ends in a handful of variables;
 * localstats (ops_localstats.c) compares every base with the window around it but knows one track only.  This operator
 * replaces every base by the correlation, covariance, slope or intercept of the two tracks over the window centred on
 * it, so that segments, binarize, histogram and statsover can go on from there.
 *
 * The track is a file of intervals read as `correlate <file>` reads it (load_track_into_partners): it is built in each
 * chromosome's partner buffer, the library writes the result over it, and the partner then becomes the signal, exactly
 * as after any out-of-place operator.  The definition is at gdsp_localcorr (include/genodsp_hip.h).
 *
 * The driver finds this operator through opgroup_localcorrelate, at the end of this file (host_services.h); every call into
 * the device library for it stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_localcorrelate)

typedef struct dspop_localcorrelate
	{
	dspop   common;
	u32     windowSize;
	int     what;
	char*   filename;
	int     valColumn, originOne;
	} dspop_localcorrelate;

static const struct { const char* name;  int what; } figures[] =
	{ { "correlation", GDSP_LOCALCORR_CORRELATION }, { "covariance", GDSP_LOCALCORR_COVARIANCE },
	  { "slope", GDSP_LOCALCORR_SLOPE }, { "intercept", GDSP_LOCALCORR_INTERCEPT } };

OP_SHORT (op_localcorrelate, "correlation of the signal with the intervals in a file over the window around each base (not in genodsp)")

void op_localcorrelate_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sReplace every base by how the signal and a second track, the values of the intervals in a\n", indent);
	fprintf (f, "%sfile (bases under no interval are 0, overlapping intervals add up), go together over the\n", indent);
	fprintf (f, "%swindow centred on it. The window is slidingsum's, cut off at the chromosome ends. Every\n", indent);
	fprintf (f, "%sstep is rounded once; for read depth the window sums are exact and so is every figure.\n", indent);
	fprintf (f, "%sNot in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s <filename> [options]\n", indent, name);
	fprintf (f, "%s  --window=<length>        (W=) window size (default: global window, else 100; at most %d);\n",
	         indent, GDSP_LOCALCORR_MAX_WINDOW);
	fprintf (f, "%s                           (W-1)/2 bases to the right, the rest to the left\n", indent);
	fprintf (f, "%s  --as=correlation         write the window's Pearson r, 0 where either track is constant\n", indent);
	fprintf (f, "%s                           (this is the default)\n", indent);
	fprintf (f, "%s  --as=covariance          write the window's population covariance\n", indent);
	fprintf (f, "%s  --as=slope               write the slope of the track regressed on the signal\n", indent);
	fprintf (f, "%s  --as=intercept           write the intercept of that regression\n", indent);
	fprintf (f, "%s  --value=<col>            intervals' values are in column <col> of the file\n", indent);
	fprintf (f, "%s  --novalue                intervals have no value; every interval counts 1\n", indent);
	fprintf (f, "%s  --origin=one|zero        intervals are origin-one, closed / origin-zero, half-open\n", indent);
	}

dspop* op_localcorrelate_parse (char* name, int argc, char** argv)
	{
	dspop_localcorrelate* op = (dspop_localcorrelate*) new_op (name, sizeof(dspop_localcorrelate), true);
	op->windowSize = (u32) get_named_global ("windowSize", 100);
	op->what       = GDSP_LOCALCORR_CORRELATION;
	op->valColumn  = (int) get_named_global ("valColumn", 4-1);
	op->originOne  = (int) get_named_global ("originOne", false);
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (is_opt3 (arg, "window", "W")) { op->windowSize = window_arg (name, arg, argVal, "window size");  continue; }
		if (strcmp_prefix (arg, "--as=") == 0)
			{
			size_t k = 0;
			while ((k < sizeof(figures)/sizeof(figures[0])) && (strcmp (argVal, figures[k].name) != 0)) k++;
			if (k == sizeof(figures)/sizeof(figures[0]))
				chastise ("[%s] --as must be correlation, covariance, slope or intercept (\"%s\")\n", name, arg);
			op->what = figures[k].what;
			continue;
			}
		if (value_column_take (name, arg, &op->valColumn)) continue;
		if (origin_opt_take (arg, &op->originOne)) continue;
		if (strcmp_prefix (arg, "--debug") == 0) continue;
		if (strcmp_prefix (arg, "--") == 0) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		if (op->filename == NULL) { op->filename = copy_string (arg);  continue; }
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->filename == NULL) chastise ("[%s] no filename was provided\n", name);
	if (op->windowSize > GDSP_LOCALCORR_MAX_WINDOW)
		chastise ("[%s] window size %u is above the largest this operator supports (%d)\n",
		          name, op->windowSize, GDSP_LOCALCORR_MAX_WINDOW);
	return (dspop*) op;
	}

void op_localcorrelate_free (dspop* _op)
	{
	dspop_localcorrelate* op = (dspop_localcorrelate*) _op;
	if (op->filename != NULL) free (op->filename);
	free (op);
	}

void op_localcorrelate_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_localcorrelate* op = (dspop_localcorrelate*) _op;
	char* name = _op->name;
	to_whole ();                                               /* the file addresses whole chromosomes */
	load_track_into_partners (name, op->filename, op->valColumn, op->originOne);

	int numChroms = 0;
	for (spec* s=chromsOfInterest ; s!=NULL ; s=s->next) numChroms++;
	gdsp_batch_item* items = (gdsp_batch_item*) must_alloc (calloc (numChroms + 1, sizeof(gdsp_batch_item)), name);
	spec**           mine  = (spec**) must_alloc (calloc (numChroms + 1, sizeof(spec*)), name);

	sync_all_devices ();                                       /* (the track is in place everywhere) */
	for (int d=0 ; d<device_count_in_use () ; d++)             /* one launch sequence per device, its chromosomes in file order */
		{
		int numMine = 0;
		for (spec* s=chromsOfInterest ; s!=NULL ; s=s->next)
			{
			if (device_index_of (s) != d) continue;
			if (trackOperations) fprintf (stderr, "%s(%s)\n", name, s->chrom);
			items[numMine].d_in = s->valVector;  items[numMine].d_out = partner_of (s);  items[numMine].n = s->length;
			mine[numMine++] = s;
			}
		if (numMine == 0) continue;
		select_device_of (mine[0]);
		check_gdsp (gdsp_localcorr_batch (items, numMine, op->windowSize, op->what, op_stream ()), name);
		for (int k=0 ; k<numMine ; k++) flip_spec (mine[k]);   /* what was the track is the signal now */
		}
	select_device_of (chromsSorted[0]);
	free (items);  free (mine);
	}

/* the driver: no traits of its own (the track is built in the partners; it is a file-driven operator on whole chromosomes) */
static const dspinfo localcorrelateRows[] =
	{ dspinforecord("localcorrelate", op_localcorrelate), dspinfoalias ("local_correlate"), dspinfoalias ("localcorrelation"),
	  dspinfoalias ("rollingcorrelation") };
const opgroup opgroup_localcorrelate = { localcorrelateRows, (int) (sizeof(localcorrelateRows)/sizeof(localcorrelateRows[0])), NULL, 0, NULL };
